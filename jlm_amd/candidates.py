"""Per-segment candidate lists behind a static decode: the host side of ``Decoder.decode_candidates``.

A decoded path cuts its input into segments, one per word.  For every segment the lattice holds the words with that start and that
end -- the *alternatives* --, and the list an input method shows under the cursor is those words ordered by the score of the path with
the segment's word replaced.  Everything the device needs of the path it finds itself in the plan's pools (``jlm_alt_frames``,
include/jlm_hip.h); from here travel one row per (sentence, segment, alternative) -- sentence, depth, word -- and the words the rows
are teacher-forced on behind the substitute.  Plain numpy: :func:`segments_of` reads a batch's traces, :func:`plan_rows` lays the
rows out, :func:`lists_of` turns the totals that come back into the lists.
"""
import numpy as np


def segments_of(lat, nodes_h, len_h, rank):
    """The segments of path ``rank`` of every sentence of ``lat`` from the decode's back-traces (``nodes_h`` [n_sent * beam, stride], the
    node ids from the last word back to the root, ``len_h`` their lengths).  -> per sentence a list of (start, end, path word id,
    alternatives' node ids) in path order, the alternatives -- every lattice node with that start and end, the path's own among them
    -- in lattice node order; [] for a sentence with fewer than rank + 1 paths."""
    B, beam = lat.n_sent, lat.beam
    out = []
    for s in range(B):
        row = s * beam + rank
        ln = int(len_h[row]) if rank < beam else 0
        segs = []
        if ln > 1:
            path = np.asarray(nodes_h[row, :ln - 1][::-1], dtype=np.int64)
            for n in path:
                start, end = int(lat.node_start[n]), int(lat.node_end[n])
                a, b = int(lat.end_off[end * B + s]), int(lat.end_off[end * B + s + 1])
                cell = np.arange(a, b, dtype=np.int64)
                segs.append((start, end, int(lat.node_word[n]), cell[lat.node_start[a:b] == start]))
        out.append(segs)
    return out


def plan_rows(lat, segments, lookahead, max_rows):
    """One row per (sentence, segment, alternative), sorted by suffix step count j = min(K - k, lookahead) (None: K - k), longest first
    (stable), so that the rows live at step t are a prefix and rows with j = 0 come last; cut into calls of at most ``max_rows`` rows --
    a segment's alternatives may fall into different calls.  -> (index [n, 3] = (sentence, segment, alternative) of every row in
    (sentence, segment, alternative) order, list of calls).  A call: dict(idx = its rows' positions in ``index``, depth, alt [R],
    sent_off [n_sent + 1], sent_rows [R], n_steps, n_live [n_steps], word, target [n_steps, R])."""
    if max_rows < 1:
        raise ValueError("max_rows must be >= 1")
    index, sent, depth, alt, steps, tails = [], [], [], [], [], []
    for s, segs in enumerate(segments):
        K = len(segs)
        words = [w for _st, _en, w, _alts in segs]
        for k, (_st, _en, _w, alts) in enumerate(segs, 1):
            j = K - k if lookahead is None else min(K - k, int(lookahead))
            for i, n in enumerate(alts):
                index.append((s, k - 1, i))
                sent.append(s)
                depth.append(k - 1)
                alt.append(int(lat.node_word[n]))
                steps.append(j)
                tails.append(words[k:k + j])
    index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
    steps = np.asarray(steps, dtype=np.int64)
    order = np.argsort(-steps, kind="stable")
    calls = []
    for i in range(0, len(order), max_rows):
        idx = order[i:i + max_rows]
        R, S = len(idx), int(steps[idx[0]])
        j = steps[idx]
        word = np.zeros((S, R), dtype=np.int32)
        target = np.zeros((S, R), dtype=np.int32)
        for r, q in enumerate(idx):
            t = tails[q]
            if len(t):
                target[:len(t), r] = t
                word[0, r] = alt[q]
                word[1:len(t), r] = t[:-1]
        sent_r = np.asarray([sent[q] for q in idx], dtype=np.int64)
        # the rows of a sentence in (segment, alternative) order: ``index`` order
        by_sent = np.lexsort((idx, sent_r))
        sent_off = np.zeros(lat.n_sent + 1, dtype=np.int32)
        np.cumsum(np.bincount(sent_r, minlength=lat.n_sent), out=sent_off[1:])
        calls.append(dict(idx=idx, depth=np.asarray([depth[q] for q in idx], dtype=np.int32),
                          alt=np.asarray([alt[q] for q in idx], dtype=np.int32), sent_off=sent_off,
                          sent_rows=by_sent.astype(np.int32), n_steps=S,
                          n_live=(j[None, :] > np.arange(S)[:, None]).sum(axis=1).astype(np.int32), word=word, target=target))
    return index, calls


def lists_of(lat, segments, index, totals, n_cand):
    """The calls' totals (``totals`` [n], parallel to ``index``) as the result: per sentence [(start, length, [(score, word), ...])] in
    path order, a segment's candidates ascending by (total, alternative order) and cut at ``n_cand``."""
    out = [[] for _ in segments]
    pos = 0
    for s, segs in enumerate(segments):
        for start, end, _w, alts in segs:
            t = totals[pos:pos + len(alts)]
            assert (index[pos:pos + len(alts), 0] == s).all()
            pos += len(alts)
            order = np.argsort(t, kind="stable")[:n_cand]
            words = lat.words_of(alts[order]).tolist()
            out[s].append((start, end - start, [(float(t[o]), w) for o, w in zip(order, words)]))
    return out
