"""`--dataset synthetic`: the bench / smoke input of SURVEY.md section 8d (not in the reference, which has no way to run
without its private data): uint8 U{0..255} / 255 images, or (rgb, depth) pairs for --model pix2pix and --model artist (256 x 256) and
--model paper_cgan / paper_sampler / paper_noise / paper_standalone / paper_baseline_standalone (65 x 65), or the 6-tuple of
--model mean_depth_estimator (65 x 65 pair, two location channels, 53 x 70 originals) and of --model experimental_sampler (the same
at 64 x 64), or the 2-, 4- or 5-tuple the `--g_arch` of --model improved_sampler reads (65 x 65 or 64 x 64)."""
from .DataPlugin import DataPlugin
from ..data import SyntheticSource, SyntheticPairSource, SyntheticEstimatorSource, SyntheticSamplerSource


DEPTH_65 = ('paper_cgan', 'paper_sampler', 'paper_noise', 'paper_standalone', 'paper_baseline_standalone')
# --model improved_sampler: --g_arch -> (crop side, entries of the tuple); an arch the model refuses gets the default pair
IMPROVED = {'A1': (65, 2), 'A2': (65, 2), 'A3': (65, 2), 'B2': (64, 2), 'D1': (64, 4), 'E1': (64, 5)}


class SyntheticDataset(DataPlugin):
    name = 'synthetic'

    @staticmethod
    def arguments():
        return {'--resize': {'type': int, 'nargs': 2, 'help': 'Image size w x h of the synthetic stream (default 32 32).'},
                '--random_crop': {'type': int, 'nargs': 2, 'help': 'Accepted so that nyuv2 configs run on synthetic pairs (always 256 x 256).'}}

    @staticmethod
    def get_source(args, sess):
        B = args.batch_size
        if args.model in ('pix2pix', 'artist'):
            return SyntheticPairSource(4, B, sess.device, 256, 1234, sess.rank), 4 * B * sess.world_size, (256, 256, 3)
        if args.model in DEPTH_65:                           # the 65x65 crops of hem/examples/paper/*/*.config
            return SyntheticPairSource(4, B, sess.device, 65, 1234, sess.rank), 4 * B * sess.world_size, (65, 65, 3)
        if args.model == 'mean_depth_estimator':
            return SyntheticEstimatorSource(4, B, sess.device, 65, (53, 70), 1234, sess.rank), 4 * B * sess.world_size, (65, 65, 3)
        if args.model == 'experimental_sampler':
            return SyntheticEstimatorSource(4, B, sess.device, 64, (53, 70), 1234, sess.rank), 4 * B * sess.world_size, (64, 64, 3)
        if args.model == 'improved_sampler':                 # the tuple the chosen --g_arch reads
            size, entries = IMPROVED.get(getattr(args, 'g_arch', 'A1'), (65, 2))
            return SyntheticSamplerSource(4, B, sess.device, size, entries, 1234, sess.rank), 4 * B * sess.world_size, (size, size, 3)
        shape = (32, 32, 3)
        if getattr(args, 'resize', None):
            shape = (args.resize[1], args.resize[0], 3)
        if getattr(args, 'grayscale', False):
            shape = shape[:2] + (1,)
        return SyntheticSource(50000, shape, B, sess.device, 1234, sess.rank), 50000, shape
