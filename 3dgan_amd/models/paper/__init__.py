"""Model plugins of the thesis experiments (the reference's hem/models/paper_*.py), discovered by the same first-base rule as
the plugins one directory up (3dgan_amd/plugins.py)."""
