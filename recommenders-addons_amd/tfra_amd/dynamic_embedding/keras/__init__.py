"""`tfra_amd.dynamic_embedding.keras` — the reference's import path of the layers (`de.keras.layers`,
PY/keras/__init__.py): the same module as `tfra_amd.dynamic_embedding.layers`, also for `import ...keras.layers` and
`from ...keras.layers import FieldWiseEmbedding`.  Nothing here depends on Keras."""
import sys

from .. import layers

sys.modules[__name__ + ".layers"] = layers

__all__ = ["layers"]
