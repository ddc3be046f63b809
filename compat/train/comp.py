"""reference train/comp.py (kmeans_compress, compressed_trained_weights) -> jlm_amd.compress

The reference reads the bit width from its command line (``--comp``) inside ``compressed_trained_weights``; here it is an argument
(default 8), and ``python -m jlm_amd.compress -e ID -c BIT`` is the command."""
from jlm_amd.compress import kmeans_compress  # noqa: F401
from jlm_amd.compress import compress_experiment as _compress_experiment


def compressed_trained_weights(experiment, debug=True, bit=8):
    return _compress_experiment(experiment, bit=bit, debug=debug)
