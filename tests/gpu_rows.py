"""Helpers of the GPU tests of the row-set drivers (tests/test_gpu_score.py, test_gpu_generate.py, test_gpu_complete.py): a fixture's
model and its oracle, ragged prompts, the log-normaliser in float64."""
import numpy as np

from jlm_amd import config as jconfig, rowsets
from jlm_amd.generate import EOS_ID
from oracle import jlm_oracle as orc

# the untied model under JLM_PRECISION=f32, whose T is the state rows (jlm_amd/rowsets.py t_is_state): no other fixture reaches
# that branch in the default suite
UNTIED_F32 = "small-untied@f32"


def load_model(root):
    jconfig.set_root(root)
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


def fixture_model(fx, name, monkeypatch):
    """-> (fixture, its model); a name "<fixture>@<precision>" loads the model under JLM_PRECISION=<precision>"""
    fixture, _, precision = name.partition("@")
    if precision:
        monkeypatch.setenv("JLM_PRECISION", precision)
    f = fx(fixture)
    model = load_model(f["root"])
    assert name != UNTIED_F32 or rowsets.t_is_state(model.dev)
    return f, model


def oracle_lm(root):
    return orc.OracleDecoder(root, 1).model


def ragged_prompts(R, V, seed, lo=1, hi=6):
    """R prompts of lo .. hi words: <eos>, then random ids in [2, V)"""
    rng = np.random.RandomState(seed)
    return [[EOS_ID] + list(rng.randint(2, V, size=rng.randint(lo, hi + 1) - 1)) for _ in range(R)]


def lse(y):
    """log sum exp of y along its last axis, in float64"""
    y = np.asarray(y, dtype=np.float64)
    m = y.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(y - m).sum(axis=-1, keepdims=True)))[..., 0]
