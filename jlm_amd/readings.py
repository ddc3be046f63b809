"""The index from a typed reading prefix to the words that begin so: ``ReadingIndex``.

A predictive keyboard asks at every keystroke which words whose reading starts with what the user has typed are likeliest here.  The
lexicon carries a reading for every word (``display/reading/POS``; synth.py:57-62 builds ``reading_dict`` by the same rule); this
module sorts the vocabulary's words by (reading, id) once, answers a prefix by bisection, and packs id lists into the bit masks that
``torch.ops.jlm.topk_rows_masked`` / ``complete_frames_masked`` (csrc/jlm_topk.hip ``topk_rows_masked_kernel``) restrict a row's
selection with.  ``LSTM_Model.predict_reading`` / ``complete_reading`` (jlm_amd/complete.py) are the callers.
"""
import bisect

import numpy as np

from .data import CharVocab

_HIRA_LO, _HIRA_HI, _HIRA_TO_KATA = 0x3041, 0x3096, 0x60


def to_katakana(text):
    """hiragana (U+3041 .. U+3096) folded to katakana (+0x60); everything else as it is.  Lexicon readings are katakana, users type
    hiragana."""
    return "".join(chr(ord(c) + _HIRA_TO_KATA) if _HIRA_LO <= ord(c) <= _HIRA_HI else c for c in text)


def reading_of(word):
    """a lexicon entry's reading: token 1 of ``display/reading/POS``, or token 0 when token 1 is empty (reading_dict's rule); None
    for an entry without three tokens (``<unk>``, ``<eos>``)"""
    tokens = word.split("/")
    if len(tokens) < 3:
        return None
    return tokens[1] if tokens[1] != "" else tokens[0]


class ReadingIndex:
    """The words of a :class:`jlm_amd.data.Vocab` sorted by (reading, id).  A CharVocab is refused: a character model's softmax is
    not over words."""

    def __init__(self, vocab):
        if isinstance(vocab, CharVocab):
            raise ValueError("a reading index needs a word vocabulary: a character model's softmax is not over words")
        pairs = []
        for i, (word, _freq) in enumerate(vocab.lexicon):
            r = reading_of(word)
            if r is not None:
                pairs.append((r, i))
        pairs.sort()
        self.V = len(vocab.lexicon)
        self.readings = [r for r, _i in pairs]
        self.ids = np.array([i for _r, i in pairs], dtype=np.int64)

    def __len__(self):
        """the number of words that have a reading"""
        return len(self.readings)

    def lookup(self, prefix, exact=False):
        """-> int64 ids, ascending, of the words whose reading starts with ``prefix`` (exact: equals it).  Hiragana is folded to
        katakana first; the empty prefix gives every word that has a reading."""
        prefix = to_katakana(prefix)
        lo = bisect.bisect_left(self.readings, prefix)
        # every reading that starts with the prefix sorts before prefix + U+10FFFF (a noncharacter: no reading holds it)
        hi = bisect.bisect_right(self.readings, prefix) if exact else bisect.bisect_left(self.readings, prefix + "\U0010ffff")
        return np.sort(self.ids[lo:hi])

    def ranges(self, prefix):
        """-> (lo, mid, hi): ``ids[lo:mid]`` are the words whose reading equals ``prefix``, ``ids[mid:hi]`` the words whose reading
        starts with it and is longer (its proper extensions), both in (reading, id) order -- contiguous because the index is sorted so.
        Hiragana is folded to katakana first.  ``Decoder.decode_predict`` sends such (lo, hi) pairs to the device, never word lists."""
        return self._ranges(to_katakana(prefix))

    def _ranges(self, prefix):
        """:meth:`ranges` of a prefix already in katakana"""
        lo = bisect.bisect_left(self.readings, prefix)
        mid = bisect.bisect_right(self.readings, prefix, lo)
        hi = bisect.bisect_left(self.readings, prefix + "\U0010ffff", mid)
        return lo, mid, hi

    def tail_spans(self, text):
        """[(s, mid, hi)] for every s in [0, len(text)) at which some word's reading properly extends text[s:]: the tail starts of an
        input whose last word is unfinished (``Decoder.decode_predict``).  The input is folded to katakana once."""
        text = to_katakana(text)
        out = []
        for s in range(len(text)):
            _lo, mid, hi = self._ranges(text[s:])
            if hi > mid:
                out.append((s, mid, hi))
        return out

    def level_table(self, max_prefix):
        """The spans of ``ids`` a word is ranked within (``LSTM_Model.rank``, include/jlm_hip.h jlm_rank_rows), for every word at once:
        -> CSR (off [V + 1], lo, hi) int32.  Word w with the reading r of n kana has the entries off[w] .. off[w + 1]: the prefix levels
        j = 0 .. min(n, max_prefix), ``ids[lo:hi]`` = the words whose reading starts with r[:j] (j = 0: every word that has a
        reading), then level X, the words whose reading equals r.  A word without a reading has no entries.  The spans of a word are
        nested (lo non-decreasing, hi non-increasing), found by bisection inside the span before.  0 <= max_prefix <= 30."""
        if isinstance(max_prefix, bool) or not isinstance(max_prefix, (int, np.integer)) or not 0 <= max_prefix <= 30:
            raise ValueError("max_prefix must be an integer in [0, 30] (got %r)" % (max_prefix,))
        rd = self.readings
        count = np.zeros(self.V, dtype=np.int64)
        spans, per_reading = {}, None
        for pos, (r, w) in enumerate(zip(rd, self.ids)):
            if pos == 0 or r != rd[pos - 1]:
                lo, hi = 0, len(rd)
                per_reading = [(lo, hi)]
                for j in range(1, min(len(r), int(max_prefix)) + 1):
                    p = r[:j]
                    lo = bisect.bisect_left(rd, p, lo, hi)
                    hi = bisect.bisect_left(rd, p + "\U0010ffff", lo, hi)
                    per_reading.append((lo, hi))
                lo = bisect.bisect_left(rd, r, lo, hi)
                per_reading.append((lo, bisect.bisect_right(rd, r, lo, hi)))
            spans[int(w)] = per_reading
            count[int(w)] = len(per_reading)
        off = np.zeros(self.V + 1, dtype=np.int64)
        np.cumsum(count, out=off[1:])
        flat = [s for w in sorted(spans) for s in spans[w]]
        both = np.asarray(flat, dtype=np.int64).reshape(-1, 2)
        return off.astype(np.int32), both[:, 0].astype(np.int32), both[:, 1].astype(np.int32)

    @staticmethod
    def mask(id_lists, V):
        """Bit masks of word-id lists: -> (uint32 [n_sets, ceil(V / 32)], the set index of each list).  Bit w & 31 of word w >> 5 of
        set s says word w is in it; equal lists share a set; bits at and beyond V stay zero.  ValueError for an id outside [0, V)."""
        ld = (int(V) + 31) // 32
        sets, rows, index = {}, [], []
        for ids in id_lists:
            a = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
            if len(a) and (a[0] < 0 or a[-1] >= V):
                raise ValueError("a word id outside [0, %d) in a word set" % V)
            key = a.tobytes()
            if key not in sets:
                sets[key] = len(rows)
                m = np.zeros(ld, dtype=np.uint32)
                np.bitwise_or.at(m, a >> 5, np.left_shift(np.uint32(1), (a & 31).astype(np.uint32)))
                rows.append(m)
            index.append(sets[key])
        out = np.stack(rows) if rows else np.zeros((0, ld), dtype=np.uint32)
        return out, np.array(index, dtype=np.int64)
