"""`hem/models/paper_baseline_standalone.py`: paper_standalone with the three versions that file offers -- `baseline`,
`mean_adjusted`, `mean_provided` -- as a plugin of its own."""
from ..ModelPlugin import ModelPlugin
from .paper_standalone import StandaloneReplica, standalone_arguments


class paper_baseline_standalone(ModelPlugin, StandaloneReplica):
    name = 'paper_baseline_standalone'

    @staticmethod
    def arguments():
        return standalone_arguments(['baseline', 'mean_adjusted', 'mean_provided'])

    def train(self, sess=None, args=None, feed_dict=None):
        return self._train()
