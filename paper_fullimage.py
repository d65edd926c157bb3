#!/usr/bin/env python3
"""Full-frame depth inference of a trained `--model paper_cgan`, `paper_standalone` or `paper_baseline_standalone` (the
thesis driver `paper_fullimage.py`): the 65x65 window slides over whole frames at each `--strides` value, the generator's
29x29 outputs are blended into a frame-sized depth map (infer_full of the model's GeneratorReplica, on the HIP kernels of
tdg_cgan_full.hip), and each (frame, stride) prints one JSON line with the
full-frame RMSE.  Unless `--no_images`, the depth, variance and montage images go to `<dir>/images/`, and the montages of
every frame at one stride are stacked into `full_montage_<s>.png` (:300-315).

Arguments are train.py's (`python paper_fullimage.py @<dir>/options.config` rebuilds the trained model) plus the flags
below.  The newest `<dir>/checkpoint-N.npz` is restored.  Frames come from the nyuv2 records of `--split` (u8 / 255 and
u16 / 65535, as the training pairs), or, with `--dataset synthetic`, from seeded 427 x 561 frames.

Deliberate differences from the reference: frames are fed in RGB order (the reference reads them
with cv2.imread, BGR, while training saw RGB); depth images are clipped to [0, 10] instead of wrapping in uint8; colours
use a piecewise-linear jet map instead of OpenCV's.
"""
import argparse
import ast
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SYNTH_H, SYNTH_W = 427, 561                     # the NYUv2 frame size
SPLITS = ('train', 'validate', 'test')


def own_parser():
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--strides', type=int, nargs='+', default=[10, 8, 6, 4, 2, 1], help='Window strides, one pass each.')
    p.add_argument('--split', default='validate', choices=SPLITS, help='Which split the frames come from.')
    p.add_argument('--frames', type=int, nargs='+', default=list(range(8)), help='Frame indices into the split.')
    p.add_argument('--offset', type=int, default=18, help='Where the 29x29 output lands in the window (reference: 18).')
    p.add_argument('--no_images', action='store_true', help='Print the JSON lines only.')
    return p


def config_tokens(path):
    """A `key value` file as argv tokens.  train.py's options.config holds Python reprs (None, [], True, (256, 256)): None,
    False and empty lists drop their flag, True leaves it bare, lists and tuples become their items."""
    out = []
    with open(path) as f:
        for line in f:
            words = line.split(None, 1)
            if not words or words[0].startswith('#') or words[0] in ('unknown_args', 'config'):
                continue
            key, raw = '--' + words[0], (words[1].strip() if len(words) > 1 else '')
            try:
                v = ast.literal_eval(raw)
            except (ValueError, SyntaxError):
                out += [key] + raw.split()
                continue
            if v is None or v is False or (isinstance(v, (list, tuple)) and not v):
                continue
            if v is True:
                out.append(key)
            elif isinstance(v, (list, tuple)):
                out += [key] + [str(x) for x in v]
            else:
                out += [key, str(v)]
    return out


MODELS = ('paper_cgan', 'paper_standalone', 'paper_baseline_standalone')      # the plugins with infer_full() and evaluate()


def parse_args(argv=None, own=None, prog='paper_fullimage', models=MODELS, check=None):
    """train.py's arguments (3dgan_amd/arguments.parse_args) plus --strides / --split / --frames / --offset / --no_images.
    `@file` arguments are expanded here, so that an options.config written by train.py parses.  `own`: another driver's
    parser of its own flags in place of own_parser() (paper_metrics.py, paper_sample_fullimage.py), `prog` its name in the
    messages, `models` the plugins it accepts and `check(args)` its further checks."""
    argv = sys.argv[1:] if argv is None else list(argv)
    expanded = []
    for a in argv:
        expanded += config_tokens(a[1:]) if a.startswith('@') else [a]
    own, rest = (own or own_parser()).parse_known_args(expanded)
    args = importlib.import_module('3dgan_amd.arguments').parse_args(rest, warn=lambda m: sys.stderr.write(m + '\n'))
    for k, v in vars(own).items():
        setattr(args, k, v)
    if args.model not in models and args.model in ('paper_sampler', 'paper_noise'):
        sampler = importlib.import_module('3dgan_amd.models.sampler.paper_sampler').SamplerReplica
        raise SystemExit('%s: %s' % (prog, sampler._WHY_NOT % ('infer_full / evaluate', args.model)))
    if args.model not in models:
        raise SystemExit('%s: --model %s only (got %r)' % (prog, ' | '.join(models), args.model))
    if any(s < 1 for s in getattr(args, 'strides', ())):
        raise SystemExit('%s: every --strides value must be >= 1' % prog)
    if check:
        check(args)
    return args


def latest_checkpoint(d):
    import glob
    import re
    best, best_n = None, -1
    for f in glob.glob(os.path.join(d, 'checkpoint-*.npz')):
        m = re.search(r'checkpoint-(\d+)\.npz$', f)
        if m and int(m.group(1)) > best_n:
            best, best_n = f, int(m.group(1))
    return best


def build_model(args):
    """The trained model: args.model with args' batch size, version and precision, restored from the newest checkpoint."""
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    ckpt = importlib.import_module('3dgan_amd.checkpoint')
    plugin = importlib.import_module('3dgan_amd.plugins').get_model(args.model)
    last = latest_checkpoint(args.dir)
    if last is None:
        raise SystemExit('paper_fullimage: no checkpoint-N.npz in %s (train with train.py --model %s first)' % (args.dir, args.model))
    args.n_gpus = 1
    sess = rt.Session(dtype=K.BF16 if args.precision == 'bf16' else K.F32, seed=args.seed or 0, rank=0, world_size=1)
    model = plugin(None, args, sess)
    ckpt.restore(last, model, sess)
    return model, last


def synthetic_frame(split, i):
    """Seeded 427 x 561 frame: image U[0,1) and depth U(0.01, 0.99), float32 (the synthetic pairs' ranges)."""
    import numpy as np
    rng = np.random.default_rng([1234, SPLITS.index(split), int(i)])
    image = rng.random((SYNTH_H, SYNTH_W, 3), dtype=np.float32)
    depth = (rng.random((SYNTH_H, SYNTH_W), dtype=np.float32) * np.float32(0.98) + np.float32(0.01)).astype(np.float32)
    return image, depth


def load_frames(args):
    """[(index, image f32 [H,W,3], depth f32 [H,W])] of args.frames in args.split."""
    import numpy as np
    if args.dataset == 'synthetic':
        return [(i,) + synthetic_frame(args.split, i) for i in args.frames]
    plugins = importlib.import_module('3dgan_amd.plugins').data_plugins()
    name = importlib.import_module('3dgan_amd.arguments').dataset_plugin_name(args.dataset)
    if name != 'nyuv2':
        raise SystemExit('paper_fullimage: --dataset nyuv2 or synthetic (got %r)' % args.dataset)
    rgb, depth = plugins[name].load(args, args.split)
    out = []
    for i in args.frames:
        if not 0 <= i < rgb.shape[0]:
            raise SystemExit('paper_fullimage: frame %d outside the %d frames of %s' % (i, rgb.shape[0], args.split))
        out.append((i, rgb[i].astype(np.float32) / np.float32(255.0), depth[i].astype(np.float32) / np.float32(65535.0)))
    return out


def jet(v):
    """Piecewise-linear jet colours of v in [0, 1] -> [..., 3] in [0, 1] (blue, cyan, yellow, red)."""
    import numpy as np
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0)[..., None]
    return np.clip(1.5 - np.abs(4.0 * v - np.array([3.0, 2.0, 1.0])), 0.0, 1.0)


def frame_images(image, depth, y_hat, g):
    """(depth, variance, montage) images in [0, 1]: predicted depth y_hat / 10 clipped to [0, 1] in jet colours, the second
    canvas -- infer_full's g (:165-212), sample_full's variance -- min-max normalised (grey), and the montage
    [image | ground truth | prediction | variance]."""
    import numpy as np
    pred = jet(np.clip(y_hat / 10.0, 0.0, 1.0))
    lo, hi = float(g.min()), float(g.max())
    var = (g - lo) / (hi - lo) if hi > lo else np.zeros_like(g)
    var = np.asarray(var, np.float64)[..., None]
    montage = np.concatenate([image, jet(depth), pred, np.repeat(var, 3, axis=2)], axis=1)
    return pred, var, montage


def sweep_frames(args, run, line, montage_name):
    """The loop of the whole-frame drivers over args.strides and args.frames.  `run(model, image, depth, stride)` returns the
    frame's result and the canvas shown as its variance image; `line(result)` is what the frame's JSON line holds between
    `patches` and `ms`; the montages of a stride are stacked into `montage_name % stride` under `<dir>/images/`."""
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
            r, second = run(model, image, depth, s)
            ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps(dict({'split': args.split, 'frame': i, 'stride': s, 'patches': r.patches}, **line(r), ms=round(ms, 3))),
                  flush=True)
            if args.no_images:
                continue
            pred, var, montage = frame_images(image, depth, r.y_hat.cpu().numpy(), second.cpu().numpy())
            stem = os.path.join(img_dir, '%s_%d_s%d_' % (args.split, i, s))
            summaries.write_png(stem + 'depth.png', pred)
            summaries.write_png(stem + 'variance.png', var)
            summaries.write_png(stem + 'montage.png', montage)
            montages.append(montage)
        if montages:
            summaries.write_png(os.path.join(img_dir, montage_name % s), np.concatenate(montages, axis=0))


def main(argv=None):
    args = parse_args(argv)

    def run(model, image, depth, s):
        r = model.infer_full(image, depth, stride=s, offset=args.offset)
        return r, r.g
    sweep_frames(args, run, lambda r: {'rmse': r.rmse}, 'full_montage_%d.png')


if __name__ == '__main__':
    main()
