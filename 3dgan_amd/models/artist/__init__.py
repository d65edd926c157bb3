"""The reference's shared-encoder RGB and depth autoencoder (hem/models/artist.py): a plugin directory of its own, scanned by
plugins.artist_model_plugins()."""
