"""Model plugins of the thesis' control experiment (hem/models/paper_standalone.py, paper_baseline_standalone.py): the depth
U-Net trained on the RMSE regression loss alone, no critic.  A plugin directory of its own: the scans of `models/`,
`models/paper/` and `models/sampler/` are pinned by their tests (3dgan_amd/plugins.py)."""
