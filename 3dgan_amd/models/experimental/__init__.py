"""The reference's experimental depth models (hem/models/experimental_sampler.py): a plugin directory of its own, scanned by
plugins.experimental_model_plugins()."""
