"""The reference's depth sampler family (hem/models/improved_sampler.py): a plugin directory of its own, scanned by
plugins.improved_model_plugins()."""
