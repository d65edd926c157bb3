"""Input pipeline entry point with the contract of the reference's `data.py:34-60`
(`get_dataset(args) -> x, x_init, x_count`) / `hem.get_dataset_tensors` (hem/util/data.py:60-100): here
`(source, count, image_shape)` where `source.next_batch()` serves this replica's batches already resident in HBM.

The dataset itself is a plugin (`3dgan_amd/data_plugins/*.py`, discovered like hem/util/data.py:11-29): cifar, mnist,
floorplan (gen-1 name: floorplans), nyuv2, synthetic.  `--resize W H` and `--grayscale` (train.py:226-231) are applied
once on the device by the image plugins.
"""
from . import plugins
from .arguments import dataset_plugin_name


def get_dataset(args, sess):
    name = dataset_plugin_name(args.dataset)
    found = plugins.data_plugins()
    if name not in found:
        raise NotImplementedError('unknown --dataset %r (available: %s)' % (args.dataset, ', '.join(sorted(found))))
    return found[name].get_source(args, sess)


SPLITS = ('train', 'validate', 'test')
SYNTH_BATCHES = 4                               # batches of a synthetic split


def open_split(args, sess, split, who='paper_metrics'):
    """(source, examples) of one split of the depth pairs: next_batch() -> (x [B,65,65,3], y [B,65,65,1]) in [0, 1] on the
    device.  A source of its own: the training source is not consumed.  `--dataset synthetic` serves seeded pairs, one stream
    per split.  `who`: the driver's name in the messages (paper_metrics.py, train.py --validation)."""
    if args.dataset == 'synthetic':
        from . import data
        src = data.SyntheticPairSource(SYNTH_BATCHES, args.batch_size, sess.device, 65, 1234 + SPLITS.index(split), sess.rank)
        return src, SYNTH_BATCHES * args.batch_size
    name = dataset_plugin_name(args.dataset)
    if name != 'nyuv2':
        raise SystemExit('%s: --dataset nyuv2 or synthetic (got %r)' % (who, args.dataset))
    if not getattr(args, 'random_crop', None) or tuple(args.random_crop) != (65, 65):
        raise SystemExit('%s: the model reads 65 x 65 crops (--random_crop 65 65)' % who)
    src, n, _ = plugins.data_plugins()[name].get_source(args, sess, split=split)
    return src, n
