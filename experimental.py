#!/usr/bin/env python3
"""The reference's top-level `experimental.py` (:29-59) on the MI355X-native hot path: ONE data source, the mean-depth estimator,
then experimental_sampler built around it; the estimator trains first, then the sampler, which reads the estimator's output and
never changes it.

    python experimental.py --dataset synthetic --batch_size 64 --estimator_epochs 30 --epochs 300 --dir workspace/experimental
    python experimental.py @examples/improved_sampler/experimental.config          (the reference's config: nyuv2 flags)

The command line is train.py's (3dgan_amd/arguments.py) with experimental_sampler's flags, the estimator's `--m_arch`, and
`--estimator_epochs` (default 30, the reference's constant at :49).  A `--model` on the command line or in a config file is
ignored: the reference's config names the estimator, the driver builds both.  `--g_arch` / `--d_arch` are forced to E2 (:43-44).
Per-epoch losses, summaries and checkpoints come from the code train.py uses (its init_run / resume / run_epochs); every
checkpoint holds the coupled model -- `generator/`, `discriminator/` and the estimator's `model/` -- so a run resumed from
--dir continues in whichever phase its epoch counter says: the estimator until `--estimator_epochs`, the sampler for `--epochs`
more.

Deviations from the reference, both deliberate:
  * `--epochs` is honoured where the reference overwrites it with 300 (:56);
  * `vargs['lr'] = 1e-4` between the phases (:57) is not reproduced: both optimizers were built before it, so it changes nothing.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import train as T                                                     # noqa: E402

SAMPLER, ESTIMATOR = 'experimental_sampler', 'mean_depth_estimator'


def parse_args(argv):
    """train.py's three-pass parse with --model experimental_sampler appended (the last --model wins), then the driver's and
    the estimator's own flags out of what that parse left over."""
    import importlib
    plugins = importlib.import_module('3dgan_amd.plugins')
    args = T._arguments().parse_args(list(argv) + ['--model', SAMPLER], warn=lambda m: None)
    extra = argparse.ArgumentParser(add_help=False)
    extra.add_argument('--estimator_epochs', type=int, default=30, help='Epochs the estimator trains before the sampler (:49).')
    for flag, spec in plugins.get_model(ESTIMATOR).arguments().items():
        if not hasattr(args, flag.lstrip('-')):
            extra.add_argument(flag, **spec)
    more, leftover = extra.parse_known_args(args.unknown_args)
    for k, v in vars(more).items():
        setattr(args, k, v)
    if leftover:
        T.message('WARNING: unknown and unused arguments provided: {}'.format(leftover))
    args.unknown_args = leftover
    args.g_arch = args.d_arch = 'E2'                                   # :43-44
    return args


def main(argv=None):
    import importlib
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    T.maybe_relaunch(args, argv, script=__file__)
    T.resolve_defaults(args)
    if args.n_gpus < 1:
        raise SystemExit('--n_gpus 0: this build has no CPU path')
    if args.estimator_epochs < 0:
        raise SystemExit('--estimator_epochs must not be negative, got %d' % args.estimator_epochs)
    sess, chief, world, x, iter_per_epoch = T.init_run(args)

    if chief:
        T.message('Initializing model...')
    plugins = importlib.import_module('3dgan_amd.plugins')
    estimator = plugins.get_model(ESTIMATOR)(x, args, sess)
    sampler = plugins.get_model(SAMPLER)(x, args, sess, estimator=estimator)
    T.resume(sampler, args, sess, chief)                               # the coupled model: all three parts

    start_time = time.time()
    epochs = int(args.epochs[1:]) if args.epochs[0] == '+' else int(args.epochs)
    for model, until in ((estimator, args.estimator_epochs), (sampler, args.estimator_epochs + epochs)):
        if chief:
            T.message('Training {} up to epoch {}...'.format(model.name, until))
        T.run_epochs(lambda s=None, a=None, m=model: m.train(s, a, None), model, args, sess, chief, iter_per_epoch, until, saved=sampler)
    T.finish(world, chief, start_time)


if __name__ == '__main__':
    main()
