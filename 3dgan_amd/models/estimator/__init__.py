"""Model plugins of the reference's second generation that estimate a scene statistic from the whole frame
(hem/models/mean_depth_estimator.py).  A plugin directory of its own: the scans of `models/`, `models/paper/` and
`models/sampler/` are pinned by their tests (3dgan_amd/plugins.py)."""
