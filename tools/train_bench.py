"""Time of a training step on the device (jlm_amd.train.DeviceStepper, csrc/jlm_train.hip): one JSON line.

  models        mid-tied and mid-vtable (V = 50 000, H = 512; E = 256 / segments 200, 100, 50), Glorot weights, dropout 0.9, self-norm
  per (model, B) at T = 20, B = 128 and 384:
                tokens/s over 50 timed steps after 10 warm-up steps, the median of three such regions (wall clock around a
                synchronised region; random ids);
                milliseconds per phase of a step by HIP events (a run of its own, 10 steps): inputs, the T forward LSTM steps, the
                vocabulary loss, the projection's backward, the T backward LSTM steps, the weight gradients and the scatter, Adam;
                the share of the 2 T sequential LSTM launches; the vocabulary products' rate (3 products of 2 N sum V_i k_i -- V E for
                a tied model --, plus the logits once more when the vocabulary takes more than one chunk; the small Q / dVT / dP
                products of a factored segment not counted) against the 157 TFLOP/s f32 matrix peak
  chunk sweep   mid-tied, B = 128: the step time with TRAIN_CHUNK_BYTES = 32, 64, 128, 256 and 512 MiB
  CPU           one float32 step of the same graph by torch autograd on this machine's CPUs (mid-tied, B = 128): what there was before
  --profile N   instead of all that: N plain steps of mid-vtable at B = 128, to be run under `rocprofv3 --kernel-trace --stats --`
  --finetune BIT [BIT ...]
                instead of all that: the codebook fine-tuning step (jlm_amd.finetune.CodebookDeviceStepper) beside the plain training
                step, IN THE SAME RUN: mid-tied and mid-vtable at B = 128, the codes of every tensor from kmeans_compress at BIT bits;
                the same warm-up, timed steps and regions for both steppers, and the fine-tuning step's phases by HIP events
                (codebook_grad, adam, expand take the place of the plain step's adam)
  --distill TEACHER_FIXTURE
                instead of all that: the distilling step (jlm_amd.distill.DistillDeviceStepper, alpha 0.5, temperature 2) beside the
                plain step of the same student, IN THE SAME RUN: student mid-tied at H = 256, teacher TEACHER_FIXTURE (mid-tied or
                mid-vtable) at H = 512, B = 128; step ms and phases of both (the phase ``teacher_forward`` ends where the teacher's P
                and Q stand; it begins after the student's LSTM, so the student's own P is inside it)

    python tools/train_bench.py [--quick] [--profile N] [--finetune BIT ...] [--distill TEACHER_FIXTURE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32_MATRIX_PEAK = 157e12
T_STEPS = 20


def _model(name, hidden=512):
    from jlm_amd import synth, train as T
    mode = name.split("-")[1]
    cfg = synth.make_config(50000, hidden, 256, mode, synth.README_SEGS, True)
    return cfg, T.init_weights(cfg, None, 101)


def _batches(V, B, n, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, V, (B, T_STEPS)), rng.randint(0, V, (B, T_STEPS))) for _ in range(n)]


def _region(st, batches, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, y in batches:
        st.step_async(x, y)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _timed(st, batches, n_warm, torch):
    """-> (the three regions' seconds, sorted; per-phase ms of a step over 10 marked steps)"""
    _region(st, batches[:n_warm], torch)
    secs = sorted(_region(st, batches, torch) for _ in range(3))
    st.losses()
    st.timed = True
    for x, y in batches[:10]:
        st.step_async(x, y)
    ph = {k: round(v / 10, 4) for k, v in st.phase_ms().items()}
    st.timed = False
    return secs, ph


def finetune_leg(bits, n_timed, n_warm, kw):
    import torch
    from jlm_amd import compress, finetune as F, train as T
    out = {"bench": "finetune", "device": torch.cuda.get_device_name(0), "num_steps": T_STEPS, "batch_size": 128, "timed_steps": n_timed,
           "warmup": n_warm, "codebook_chunk": F.CODEBOOK_CHUNK}
    for name in ("mid-tied", "mid-vtable"):
        cfg, w = _model(name)
        batches = _batches(50000, 128, n_timed)
        st = T.DeviceStepper(cfg, w, 128, T_STEPS, **kw)
        secs, ph = _timed(st, batches, n_warm, torch)
        plain_ms = secs[1] / n_timed * 1e3
        out["%s plain" % name] = {"step_ms": round(plain_ms, 3), "regions_s": [round(s, 4) for s in secs], "phase_ms": ph,
                                  "parameters": int(sum(n for _k, _i, _s, _o, n in st.layout))}
        del st
        torch.cuda.empty_cache()
        for bit in bits:
            t0 = time.perf_counter()
            pairs = {k: compress.kmeans_compress(v, bit) for k, v in w.items()}
            t1 = time.perf_counter()
            st = F.CodebookDeviceStepper(cfg, {k: c for k, (c, _b) in pairs.items()}, {k: b for k, (_c, b) in pairs.items()}, 128, T_STEPS, **kw)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            secs, ph = _timed(st, batches, n_warm, torch)
            step_ms = secs[1] / n_timed * 1e3
            out["%s %d bit" % (name, bit)] = {
                "step_ms": round(step_ms, 3), "plain_step_ms": round(plain_ms, 3), "ratio": round(step_ms / plain_ms, 4),
                "regions_s": [round(s, 4) for s in secs], "phase_ms": ph, "groups": st.n_groups, "chunks": st.n_chunks,
                "compress_s": round(t1 - t0, 3), "stepper_setup_s": round(t2 - t1, 3)}
            del st
            torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


def distill_leg(teacher_name, n_timed, n_warm, kw, alpha=0.5, temperature=2.0):
    import torch
    from jlm_amd import distill as D, train as T
    cfg, w = _model("mid-tied", 256)
    tcfg, tw = _model(teacher_name)
    batches = _batches(50000, 128, n_timed)
    out = {"bench": "distill", "device": torch.cuda.get_device_name(0), "num_steps": T_STEPS, "batch_size": 128, "timed_steps": n_timed,
           "warmup": n_warm, "chunk_bytes": T.TRAIN_CHUNK_BYTES, "student": "mid-tied H=256", "teacher": "%s H=512" % teacher_name,
           "alpha": alpha, "temperature": temperature}
    for leg in ("plain", "distill"):
        if leg == "plain":
            st = T.DeviceStepper(cfg, w, 128, T_STEPS, **kw)
        else:
            st = D.DistillDeviceStepper(cfg, w, tcfg, tw, 128, T_STEPS, alpha=alpha, temperature=temperature, **kw)
        secs, ph = _timed(st, batches, n_warm, torch)
        out[leg] = {"step_ms": round(secs[1] / n_timed * 1e3, 3), "regions_s": [round(s, 4) for s in secs], "phase_ms": ph,
                    "words_per_window": st.Vc, "vocab_windows": -(-st.d["V"] // st.Vc)}
        del st
        torch.cuda.empty_cache()
    out["ratio"] = round(out["distill"]["step_ms"] / out["plain"]["step_ms"], 4)
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="10 timed steps per region, B = 128 only")
    ap.add_argument("--profile", type=int, default=0, metavar="N")
    ap.add_argument("--finetune", type=int, nargs="+", default=None, metavar="BIT")
    ap.add_argument("--distill", default=None, metavar="TEACHER_FIXTURE", choices=("mid-tied", "mid-vtable"))
    args = ap.parse_args(argv)
    import torch
    from jlm_amd import train as T
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=1)
    if args.finetune:
        return finetune_leg(args.finetune, *((10, 3) if args.quick else (50, 10)), kw)
    if args.distill:
        return distill_leg(args.distill, *((10, 3) if args.quick else (50, 10)), kw)
    if args.profile:
        cfg, w = _model("mid-vtable")
        st = T.DeviceStepper(cfg, w, 128, T_STEPS, **kw)
        for x, y in _batches(50000, 128, args.profile):
            st.step_async(x, y)
        st.losses()
        return None
    n_timed, n_warm = (10, 3) if args.quick else (50, 10)
    out = {"bench": "train", "device": torch.cuda.get_device_name(0), "num_steps": T_STEPS, "timed_steps": n_timed, "warmup": n_warm,
           "chunk_bytes": T.TRAIN_CHUNK_BYTES}
    for name in ("mid-tied", "mid-vtable"):
        cfg, w = _model(name)
        for B in ((128,) if args.quick else (128, 384)):
            N = B * T_STEPS
            st = T.DeviceStepper(cfg, w, B, T_STEPS, **kw)
            batches = _batches(50000, B, n_timed)
            _region(st, batches[:n_warm], torch)
            secs = sorted(_region(st, batches, torch) for _ in range(3))
            st.losses()
            st.timed = True
            for x, y in batches[:10]:
                st.step_async(x, y)
            ph = {k: round(v / 10, 4) for k, v in st.phase_ms().items()}
            st.timed = False
            step_ms = sum(ph.values())
            n_chunks = -(-st.d["V"] // st.Vc)
            vk = sum((sg[1] - sg[0]) * sg[2] for sg in st.segs)          # sum V_i k_i: V E for a tied model, the factored cost for V_table
            flops = (3 + (1 if n_chunks > 1 else 0)) * 2.0 * N * vk
            out["%s B=%d" % (name, B)] = {
                "tokens_per_s": round(N * n_timed / secs[1]), "step_ms": round(secs[1] / n_timed * 1e3, 3),
                "regions_s": [round(s, 4) for s in secs], "phase_ms": ph, "vocab_chunks": n_chunks, "vocabulary_GFLOP": round(flops / 1e9, 1),
                "lstm_share": round((ph["lstm_forward"] + ph["lstm_backward"]) / step_ms, 4),
                "vocabulary_TFLOP_per_s": round(flops / (ph["vocabulary"] * 1e-3) / 1e12, 3),
                "vocabulary_of_f32_matrix_peak": round(flops / (ph["vocabulary"] * 1e-3) / F32_MATRIX_PEAK, 4)}
            del st
            torch.cuda.empty_cache()
    cfg, w = _model("mid-tied")
    sweep = {}
    for mib in (32, 64, 128, 256, 512):
        st = T.DeviceStepper(cfg, w, 128, T_STEPS, chunk_bytes=mib << 20, **kw)
        batches = _batches(50000, 128, 10)
        _region(st, batches[:3], torch)
        secs = sorted(_region(st, batches, torch) for _ in range(3))
        sweep["%d MiB" % mib] = {"words_per_chunk": st.Vc, "step_ms": round(secs[1] / 10 * 1e3, 3)}
        del st
        torch.cuda.empty_cache()
    out["chunk_sweep mid-tied B=128"] = sweep
    try:
        from tests import train_cases as tc
        torch.set_num_threads(min(16, torch.get_num_threads()))
        x, y = _batches(50000, 128, 1)[0]
        m_in, m_out = T.dropout_mask(1, 0, 0, (2560, 256), 0.9), T.dropout_mask(1, 0, 1, (2560, 512), 0.9)
        z = np.zeros((128, 512))
        t0 = time.perf_counter()
        tc.torch_grads(cfg, w, x, y, z, z, m_in, m_out, 0.1, dtype=torch.float32)
        dt = time.perf_counter() - t0
        out["cpu_torch_f32 mid-tied B=128"] = {"threads": torch.get_num_threads(), "step_s": round(dt, 3), "tokens_per_s": round(2560 / dt)}
    except ImportError:
        out["cpu_torch_f32 mid-tied B=128"] = "tests/train_cases.py is not importable here: not measured"
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
