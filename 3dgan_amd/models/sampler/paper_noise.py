"""`hem/models/paper_noise.py` (arguments :15-48): paper_sampler's `x` case -- the noise channel beside the generator's RGB
input, no batch norm in the encoder -- as a plugin of its own, with the reference's one-choice `--model_version baseline`
(which is paper_cgan's mean_adjusted model, :93-96)."""
from ..ModelPlugin import ModelPlugin
from .paper_sampler import SamplerReplica, rate_arguments


class paper_noise(ModelPlugin, SamplerReplica):
    name = 'paper_noise'

    @staticmethod
    def arguments():
        a = rate_arguments()
        a['--model_version'] = {'type': str, 'default': 'baseline', 'choices': ['baseline'], 'help': 'Which version of the model to run.'}
        return a

    @staticmethod
    def noise_layer(args):
        return 'x'

    @staticmethod
    def encoder_batch_norm(args):
        return False

    def train(self, sess=None, args=None, feed_dict=None):
        return self._train()
