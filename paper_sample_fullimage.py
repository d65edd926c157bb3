#!/usr/bin/env python3
"""Whole-frame uncertainty maps of a trained `--model paper_sampler` or `paper_noise`: the 65x65 window slides over whole
frames at each `--strides` value, every window runs through the sampler pass -- a batch of copies of that one window, one
noise draw per copy -- and the per-pixel mean and variance of the draws are blended into frame canvases
(SamplerReplica.sample_full, on the HIP kernels of tdg_cgan_full_sample.hip and tdg_cgan_full.hip).  Each (frame, stride)
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
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from paper_fullimage import SPLITS, config_tokens, latest_checkpoint, build_model, load_frames, jet, synthetic_frame  # noqa: E402,F401

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


def parse_args(argv=None):
    """train.py's arguments plus the flags of own_parser(); `@file` arguments are expanded as paper_fullimage.py expands them."""
    argv = sys.argv[1:] if argv is None else list(argv)
    expanded = []
    for a in argv:
        expanded += config_tokens(a[1:]) if a.startswith('@') else [a]
    own, rest = own_parser().parse_known_args(expanded)
    args = importlib.import_module('3dgan_amd.arguments').parse_args(rest, warn=lambda m: sys.stderr.write(m + '\n'))
    for k, v in vars(own).items():
        setattr(args, k, v)
    if args.model not in MODELS:
        raise SystemExit('%s: --model %s only (got %r)' % (PROG, ' | '.join(MODELS), args.model))
    if any(s < 1 for s in args.strides):
        raise SystemExit('%s: every --strides value must be >= 1' % PROG)
    if args.draws is not None and (args.draws < 1 or args.batch_size % args.draws):
        raise SystemExit('%s: --draws %d must divide --batch_size %d' % (PROG, args.draws, args.batch_size))
    return args


def frame_images(image, depth, y_hat, var):
    """(depth, variance, montage) images in [0, 1]: predicted depth y_hat / 10 clipped to [0, 1] in jet colours, the variance
    canvas min-max normalised (grey), and the montage [image | ground truth | prediction | variance]."""
    import numpy as np
    pred = jet(np.clip(y_hat / 10.0, 0.0, 1.0))
    lo, hi = float(var.min()), float(var.max())
    grey = (var - lo) / (hi - lo) if hi > lo else np.zeros_like(var)
    grey = np.asarray(grey, np.float64)[..., None]
    montage = np.concatenate([image, jet(depth), pred, np.repeat(grey, 3, axis=2)], axis=1)
    return pred, grey, montage


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    summaries = importlib.import_module('3dgan_amd.summaries')
    frames = load_frames(args)
    model, last = build_model(args)
    img_dir = os.path.join(args.dir, 'images')
    if not args.no_images:
        os.makedirs(img_dir, exist_ok=True)
    for s in args.strides:
        montages = []
        for i, image, depth in frames:
            t0 = time.perf_counter()
            r = model.sample_full(image, depth, stride=s, offset=args.offset, draws=args.draws)
            ms = (time.perf_counter() - t0) * 1e3
            H, W = r.var.shape
            var_mean = float(r.var[18:H - 46, 18:W - 46].double().mean().item())
            print(json.dumps({'split': args.split, 'frame': i, 'stride': s, 'patches': r.patches, 'draws': r.draws, 'rmse': r.rmse,
                              'err_mean': r.err_mean, 'err_min': r.err_min, 'var_mean': var_mean, 'ms': round(ms, 3)}), flush=True)
            if args.no_images:
                continue
            pred, grey, montage = frame_images(image, depth, r.y_hat.cpu().numpy(), r.var.cpu().numpy())
            stem = os.path.join(img_dir, '%s_%d_s%d_' % (args.split, i, s))
            summaries.write_png(stem + 'depth.png', pred)
            summaries.write_png(stem + 'variance.png', grey)
            summaries.write_png(stem + 'montage.png', montage)
            montages.append(montage)
        if montages:
            summaries.write_png(os.path.join(img_dir, 'sample_montage_%d.png' % s), np.concatenate(montages, axis=0))


if __name__ == '__main__':
    main()
