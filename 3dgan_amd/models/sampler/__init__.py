"""Model plugins of the thesis' second experiment (hem/models/paper_sampler.py, paper_noise.py): the depth cGAN with one
channel of uniform noise at a node of the generator, and the sampler statistics.  A plugin directory of its own: the scans of
`models/` and `models/paper/` are pinned by their tests (3dgan_amd/plugins.py)."""
