"""Plugin discovery with the semantics of the reference's gen-2 registry (`hem/util/data.py:11-29`,
`hem/models/ModelPlugin.py:4-8`): every `*.py` in a plugin directory is imported and every class DEFINED in that module
whose FIRST base class is named `ModelPlugin` / `DataPlugin` is registered under its `name` attribute.  So dropping a
new file into `3dgan_amd/models/` or `3dgan_amd/data_plugins/` is all it takes to add `--model foo` / `--dataset foo`
(and its `arguments()` to the command line: 3dgan_amd/arguments.py).
"""
import importlib
import inspect
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def search_for_plugins(plugin_dir, plugin_module, plugin_name):
    """hem/util/data.py:11-29."""
    valid = []
    files = sorted(f for f in os.listdir(plugin_dir) if f.endswith('.py') and f not in ('__init__.py', plugin_name + '.py'))
    for f in files:
        module_name = plugin_module + '.' + f[:-3]
        mod = importlib.import_module(module_name)
        for _, cls in inspect.getmembers(mod, inspect.isclass):
            if cls.__module__ == module_name and cls.__bases__ and cls.__bases__[0].__name__ == plugin_name:
                valid.append(cls)
    return {cls.name: cls for cls in valid}


def model_plugins():
    return search_for_plugins(os.path.join(_HERE, 'models'), '3dgan_amd.models', 'ModelPlugin')


def paper_model_plugins():
    """The thesis experiments (hem/models/paper_*.py) have a plugin directory of their own, `3dgan_amd/models/paper/`."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'paper'), '3dgan_amd.models.paper', 'ModelPlugin')


def sampler_model_plugins():
    """The thesis' noise / sampler experiment (hem/models/paper_sampler.py, paper_noise.py): `3dgan_amd/models/sampler/`."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'sampler'), '3dgan_amd.models.sampler', 'ModelPlugin')


def standalone_model_plugins():
    """The thesis' control experiment (hem/models/paper_standalone.py, paper_baseline_standalone.py):
    `3dgan_amd/models/standalone/`.  Not part of all_model_plugins(), whose result is pinned; get_model() looks here too."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'standalone'), '3dgan_amd.models.standalone', 'ModelPlugin')


def estimator_model_plugins():
    """The scene mean-depth regressor (hem/models/mean_depth_estimator.py): `3dgan_amd/models/estimator/`.  Like the standalone
    directory it stays out of all_model_plugins(), whose result is pinned."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'estimator'), '3dgan_amd.models.estimator', 'ModelPlugin')


def experimental_model_plugins():
    """The depth cGAN fed by the estimator (hem/models/experimental_sampler.py): `3dgan_amd/models/experimental/`.  It stays out
    of every_model_plugin(), whose result is pinned like all_model_plugins()'s; known_model_plugins() adds it."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'experimental'), '3dgan_amd.models.experimental', 'ModelPlugin')


def every_model_plugin():
    """all_model_plugins(), the standalone directory and the estimator directory."""
    found = all_model_plugins()
    found.update(standalone_model_plugins())
    found.update(estimator_model_plugins())
    return found


def known_model_plugins():
    """every_model_plugin() and the experimental directory (pinned; `--model` accepts accepted_model_plugins())."""
    found = every_model_plugin()
    found.update(experimental_model_plugins())
    return found


def improved_model_plugins():
    """The depth sampler family A1-A3, B2, D1, E1 (hem/models/improved_sampler.py): `3dgan_amd/models/improved/`.  It stays out
    of known_model_plugins(), whose result is pinned like the other two unions'; accepted_model_plugins() adds it."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'improved'), '3dgan_amd.models.improved', 'ModelPlugin')


def accepted_model_plugins():
    """known_model_plugins() and the improved directory (pinned; `--model` accepts trainable_model_plugins())."""
    found = known_model_plugins()
    found.update(improved_model_plugins())
    return found


def artist_model_plugins():
    """The shared-encoder RGB and depth autoencoder (hem/models/artist.py): `3dgan_amd/models/artist/`.  It stays out of
    accepted_model_plugins(), whose result is pinned like the unions before it; trainable_model_plugins() adds it."""
    return search_for_plugins(os.path.join(_HERE, 'models', 'artist'), '3dgan_amd.models.artist', 'ModelPlugin')


def trainable_model_plugins():
    """accepted_model_plugins() and the artist directory: what `--model` accepts."""
    found = accepted_model_plugins()
    found.update(artist_model_plugins())
    return found


def all_model_plugins():
    """Every `--model` plugin: the three directories."""
    found = model_plugins()
    found.update(paper_model_plugins())
    found.update(sampler_model_plugins())
    return found


def data_plugins():
    return search_for_plugins(os.path.join(_HERE, 'data_plugins'), '3dgan_amd.data_plugins', 'DataPlugin')


def get_model(name):
    """hem/models/ModelPlugin.py:4-8: the plugin class registered under `name` (KeyError for an unknown name, as there)."""
    return trainable_model_plugins()[name]


def get_dataset(name):
    """hem/util/data.py:32-35."""
    return data_plugins()[name]
