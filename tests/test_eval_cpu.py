"""CPU-only: the eval harness (jlm_amd/eval.py) reproduces the hit counts and log
body captured from the reference's eval.py (tests/golden/eval.json), and compat/
gives a script written against the reference's module names jlm_amd's classes.
Device kernels are doubled by tests/fake_hip.py; the same harness is exercised on
the GPU in test_gpu_eval.py."""
import contextlib
import io
import os

import pytest

from jlm_amd import config as jconfig, synth
from tests import fake_hip
from tests import golden_cases as gc


def _prepare(fx, fixture):
    f = fx(fixture)
    synth.write_test_corpus(f["root"], f["lexicon"], f["cfg"]["vocab_size"], **gc.EVAL_CORPUS)
    jconfig.set_root(f["root"])
    return f


def _body(path):
    with open(path, "r", encoding="utf-8") as fh:
        body = fh.read()
    return body[:body.index("--- ")] if "--- " in body else body


@pytest.mark.parametrize("case", gc.EVAL_CASES, ids=[c[0] for c in gc.EVAL_CASES])
@pytest.mark.parametrize("batch", [1, 8])
def test_eval_harness_matches_reference(case, batch, fx, golden_eval, monkeypatch, tmp_path):
    name, fixture, argv = case
    fake_hip.install(monkeypatch)
    _prepare(fx, fixture)
    monkeypatch.chdir(tmp_path)
    from jlm_amd import eval as jeval
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        jeval.main(argv + ["--batch", str(batch)])
    gold = golden_eval[name]
    assert [ln for ln in buf.getvalue().splitlines() if ln.startswith("best_hit")] == gold["stdout_hits"]
    assert _body(os.path.join("eval", gold["log_name"])) == gold["log_body"]


# the imports of the reference's decoder/eval.py by bare module name (compat/README.md), then what each name must resolve to
COMPAT_SCRIPT = """
import config
from decoder import Decoder, CharRNNDecoder
from decoder_dynamic import DynamicDecoder
from decoder_ngram import NGramDecoder
from model import LSTM_Model
from model_ngram import NGramModel
from train.data import Vocab, CharVocab
import jlm_amd.config, jlm_amd.data, jlm_amd.decoder, jlm_amd.decoder_char, jlm_amd.decoder_dynamic, jlm_amd.decoder_ngram
import jlm_amd.model, jlm_amd.model_ngram
from jlm_amd import synth
assert config.data_path == jlm_amd.config.data_path
assert issubclass(Decoder, jlm_amd.decoder.Decoder) and issubclass(CharRNNDecoder, jlm_amd.decoder_char.CharRNNDecoder)
assert issubclass(DynamicDecoder, jlm_amd.decoder_dynamic.DynamicDecoder)
assert (NGramDecoder, LSTM_Model, NGramModel) == (jlm_amd.decoder_ngram.NGramDecoder, jlm_amd.model.LSTM_Model, jlm_amd.model_ngram.NGramModel)
assert (Vocab, CharVocab) == (jlm_amd.data.Vocab, jlm_amd.data.CharVocab)
sents = synth.make_sentences(4, 6, seed=1, alphabet=ALPHABET)
for compat_cls, cls, kw in ((Decoder, jlm_amd.decoder.Decoder, {}), (DynamicDecoder, jlm_amd.decoder_dynamic.DynamicDecoder, {"vocab_select": True})):
    dec = compat_cls(1)
    assert dec.perf_timing
    assert dec.decode_batch(sents, beam_width=5, **kw) == cls(1).decode_batch(sents, beam_width=5, **kw)
"""


def test_compat_modules_resolve_to_jlm_amd(fx, monkeypatch, tmp_path):
    """compat/ as tools/run_reference_eval.py sets it up (compat/ first on sys.path, the script run as __main__): every module name the
    reference's eval.py imports gives jlm_amd's class, and the decoders decode as jlm_amd's with per-frame timing on (eval.py prints
    their perf_log_* lists)"""
    import sys
    from tools import run_reference_eval
    fake_hip.install(monkeypatch)
    monkeypatch.setattr(sys, "path", list(sys.path))
    f = fx("small-tied")
    jconfig.set_root(f["root"])
    script = tmp_path / "uses_compat.py"
    script.write_text(COMPAT_SCRIPT.replace("ALPHABET", str(f["alphabet"])), encoding="utf-8")
    with contextlib.redirect_stdout(io.StringIO()):
        run_reference_eval.run(str(script), [])
