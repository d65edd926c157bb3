#!/usr/bin/env python3
"""Whole-frame uncertainty maps of a trained `--model paper_sampler` or `paper_noise`: the 65x65 window slides over whole
frames at each `--strides` value, every window runs through the sampler pass -- a batch of copies of that one window, one
noise draw per copy -- and the per-pixel mean and variance of the draws are blended into frame canvases
(SamplerReplica.sample_full, on the HIP kernels of tdg_cgan_full.hip).  Each (frame, stride)
prints one JSON line: split, frame, stride, patches, draws, rmse (the frame RMSE of the mean prediction), err_mean / err_min
(the mean over the windows of the mean / min over the draws of the per-draw mean absolute error), var_mean (the variance
canvas averaged over the RMSE region) and ms.  Unless `--no_images`, `<dir>/images/` receives per frame `*_depth.png`,
`*_variance.png` (the variance canvas -- a real variance, unlike paper_fullimage.py's min-max normalised g -- min-max normalised,
grey) and `*_montage.png` [image | truth | prediction | variance], and per stride `sample_montage_<s>.png`.

Arguments are train.py's (`python paper_sample_fullimage.py @<dir>/options.config` rebuilds the trained model) plus the flags
below; the newest `<dir>/checkpoint-N.npz` is restored and the frames come from where paper_fullimage.py takes them.  The
reference has no such driver: its paper_fullimage.py:317 stops at a commented-out block for the sampler model.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import paper_fullimage as pf  # noqa: E402
from paper_fullimage import SPLITS, config_tokens, latest_checkpoint, build_model, load_frames, jet, synthetic_frame, frame_images  # noqa: E402,F401

MODELS = ('paper_sampler', 'paper_noise')
PROG = 'paper_sample_fullimage'


def own_parser():
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--strides', type=int, nargs='+', default=[10], help='Window strides, one sweep each.')
    p.add_argument('--split', default='validate', choices=SPLITS, help='Which split the frames come from.')
    p.add_argument('--frames', type=int, nargs='+', default=list(range(8)), help='Frame indices into the split.')
    p.add_argument('--offset', type=int, default=18, help='Where the 29x29 output lands in the window (reference: 18).')
    p.add_argument('--draws', type=int, default=None,
                   help='Noise draws per window (default: the batch size; must divide it, and equal it with encoder batch norm).')
    p.add_argument('--no_images', action='store_true', help='Print the JSON lines only.')
    return p


def check_draws(args):
    if args.draws is not None and (args.draws < 1 or args.batch_size % args.draws):
        raise SystemExit('%s: --draws %d must divide --batch_size %d' % (PROG, args.draws, args.batch_size))


def parse_args(argv=None):
    """train.py's arguments plus the flags of own_parser(), through paper_fullimage.py's argument handling."""
    return pf.parse_args(argv, own=own_parser(), prog=PROG, models=MODELS, check=check_draws)


def main(argv=None):
    args = parse_args(argv)

    def run(model, image, depth, s):
        r = model.sample_full(image, depth, stride=s, offset=args.offset, draws=args.draws)
        return r, r.var

    def line(r):
        H, W = r.var.shape
        var_mean = float(r.var[18:H - 46, 18:W - 46].double().mean().item())
        return {'draws': r.draws, 'rmse': r.rmse, 'err_mean': r.err_mean, 'err_min': r.err_min, 'var_mean': var_mean}
    pf.sweep_frames(args, run, line, 'sample_montage_%d.png')


if __name__ == '__main__':
    main()
