"""reference train/train.py (``parameters``, ``train_RNNLM``) -> jlm_amd.train

The reference hands ``parameters`` to sacred and trains under ``@ex.automain``; here the dict is edited in place and
``train_RNNLM()`` (or running this file) trains it on the device: ``python -m jlm_amd.train --key value ...`` is the command."""
from jlm_amd.train import DEFAULTS as _DEFAULTS
from jlm_amd.train import train_experiment as _train_experiment

parameters = dict(_DEFAULTS)


def train_RNNLM(root=None):
    return _train_experiment(parameters, root=root)


if __name__ == "__main__":
    train_RNNLM()
