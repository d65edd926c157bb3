#!/usr/bin/env python3
"""Dataset evaluation of a trained `--model paper_cgan`, `paper_standalone` or `paper_baseline_standalone` (the thesis driver `paper/paper_metrics.py`): for each split, the
Eigen-2014 metrics of the model next to the two trivial predictors it has to beat, the split's mean depth image and g = 0,
each averaged over the split's batches (paper_cgan.evaluate, on the HIP kernels of tdg_cgan_eval.hip).  Per split: the
three blocks in the reference's key order, one JSON line, `<dir>/metrics/<split>.json` and, unless `--no_images`,
`<split>_mean.png`, `<split>_mean_colorized.png` and `<split>_var.png`.

Arguments are train.py's (`python paper_metrics.py @<dir>/options.config --dir <dir>` rebuilds the trained model) plus the
flags below; the newest `<dir>/checkpoint-N.npz` is restored (paper_fullimage.py's argument handling).  `--dataset
synthetic` evaluates seeded 65x65 pairs, one stream per split.

Deliberate differences from the reference: the means are plain float64 means, so NaN / inf stay
visible (the reference sums dicts with collections.Counter, whose `+` drops entries that are not positive); one replica and
the newest checkpoint instead of two towers and `checkpoint-50`; the mean image is clipped to [0, 1] instead of wrapping in
uint8; `zero` shares the model sweep's batches.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import paper_fullimage as pf  # noqa: E402

SPLITS = pf.SPLITS
SYNTH_BATCHES = 4                               # batches of a synthetic split
# paper_metrics.py:129: the printed order and names
REPORT_KEYS = (('t1', 'threshold1'), ('t2', 'threshold2'), ('t3', 'threshold3'), ('abs_rel_diff', 'abs_rel_diff'),
               ('squared_rel_diff', 'squared_rel_diff'), ('linear_rmse', 'linear_rmse'), ('log_rmse', 'log_rmse'),
               ('scale_invariant_log_rmse', 'scale_invariant_log_rmse'))
BLOCKS = (('Model metrics:', 'model'), ('Mean metrics:', 'mean'), ('Zero metrics:', 'zero'))


def own_parser():
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--splits', nargs='+', default=['validate', 'train'], choices=SPLITS, help='Splits to evaluate, in order.')
    p.add_argument('--n_batches', type=int, default=None, help='Batches per sweep (default: split size // batch size).')
    p.add_argument('--no_images', action='store_true', help='Write no PNG files.')
    return p


def parse_args(argv=None):
    args = pf.parse_args(argv, own=own_parser(), prog='paper_metrics')
    if args.n_batches is not None and args.n_batches < 1:
        raise SystemExit('paper_metrics: --n_batches must be >= 1')
    return args


def open_split(args, sess, split):
    """(source, examples) of one split: next_batch() -> (x [B,65,65,3], y [B,65,65,1]) in [0, 1] on the device."""
    return importlib.import_module('3dgan_amd.datasets').open_split(args, sess, split, who='paper_metrics')


def batches_of(args, examples):
    return args.n_batches if args.n_batches is not None else max(1, examples // args.batch_size)


def format_block(title, values):
    """One block of the reference's report (:128-130): the title, then a tab, the key and three decimals per line."""
    return '\n'.join([title] + ['\t{}: {:.3f}'.format(k, values[src]) for k, src in REPORT_KEYS])


def format_report(result):
    return '\n'.join(format_block(title, result[key]) for title, key in BLOCKS)


def record(split, checkpoint, result):
    """What `<split>.json` and the JSON line hold: evaluate()'s scalars (the images go to the PNG files)."""
    out = {'split': split, 'checkpoint': os.path.basename(checkpoint), 'n_batches': result['n_batches'], 'images': result['images']}
    out.update({k: result[k] for k in ('model', 'zero', 'mean')})
    return out


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    summaries = importlib.import_module('3dgan_amd.summaries')
    model, last = pf.build_model(args)
    out_dir = os.path.join(args.dir, 'metrics')
    os.makedirs(out_dir, exist_ok=True)
    for split in args.splits:
        source, examples = open_split(args, model.sess, split)
        result = model.evaluate(source, batches_of(args, examples))
        print('Calculating metrics for {} set...'.format(split))
        print(format_report(result), flush=True)
        rec = record(split, last, result)
        print(json.dumps(rec), flush=True)
        with open(os.path.join(out_dir, split + '.json'), 'w') as f:
            json.dump(rec, f, indent=1)
        if args.no_images:
            continue
        mean = np.clip(result['mean_image'], 0.0, 1.0)
        summaries.write_png(os.path.join(out_dir, split + '_mean.png'), mean)
        summaries.write_png(os.path.join(out_dir, split + '_mean_colorized.png'), pf.jet(mean))
        summaries.write_png(os.path.join(out_dir, split + '_var.png'), np.clip(result['var_image'], 0.0, 1.0))


if __name__ == '__main__':
    main()
