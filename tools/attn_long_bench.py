#!/usr/bin/env python3
"""Time the long-utterance attention forward (ob_relattn_infer, csrc/relattn_long.hip) next to
what runs without it: the torch core MHSA.forward falls back to past T' = 512 (restated here
from onebit_asr/conformer.py, MHSA.forward after the projections: heads view, content and
position products, rel_shift, scale, mask, softmax, nan_to_num, A v, back to [B, T, H*d]) and, at
T' = 512, the fused forward without saved state (ob_relattn_fwd, saved = NULL, p = 0).

Shapes at H = 4, d = 36: B = 8 at T' = 512, 640, 874, 1024; B = 2 at 2048; B = 1 at 4096; and
B = 8, T' = 874 at d = 64. Full lengths. Every shape is warmed first; the sides alternate within
the process, each window device events around enough repetitions for --window-ms; the medians of
--rounds windows are reported, one JSON line per shape: us per call of each side, the ratios, ps
per query-key pair of both kernels, and max |infer - torch| as a check that the sides compute
the same thing.

Usage: python tools/attn_long_bench.py [--rounds 5] [--window-ms 60] [--out FILE]"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd")]

import torch  # noqa: E402

from onebit_asr import _lib  # noqa: E402
from onebit_asr.conformer import rel_shift  # noqa: E402

SHAPES = [(8, 512, 4, 36), (8, 640, 4, 36), (8, 874, 4, 36), (8, 1024, 4, 36), (2, 2048, 4, 36),
          (1, 4096, 4, 36), (8, 874, 4, 64)]  # (B, T', H, d)


def torch_core(q, k, v, pos, u, vb, mask, H):
    """MHSA.forward's fallback between the projections and out_proj (eval: dropout is identity)."""
    bsz, tlen, width = q.shape
    d = width // H
    heads = lambda x, n: x.view(n, -1, H, d).transpose(1, 2)  # noqa: E731
    qh, kh, vh = heads(q, bsz), heads(k, bsz), heads(v, bsz)
    content = torch.matmul(qh + u.view(1, H, 1, d), kh.transpose(-2, -1))
    p = heads(pos, 1)
    position = rel_shift(torch.matmul(qh + vb.view(1, H, 1, d), p.transpose(-2, -1)))
    scores = (content + position) / math.sqrt(d)
    scores = scores.masked_fill(mask[:, None, :, :] == 0, float("-inf"))
    attn = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)
    return torch.matmul(attn, vh).transpose(1, 2).contiguous().view(bsz, tlen, width)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    kc = int(lib.ob_relattn_infer_key_chunk())

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    for B, T, H, d in SHAPES:
        C = H * d
        g = torch.Generator(device=dev).manual_seed(T + d)
        q, k, v = (torch.randn(B, T, C, device=dev, generator=g) for _ in range(3))
        pos = torch.randn(1, T, C, device=dev, generator=g)
        u, vb = (torch.randn(H, d, device=dev, generator=g) * 0.01 for _ in range(2))
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        mask = torch.ones(B, T, T, dtype=torch.bool, device=dev)
        ctx, ctx_f = torch.empty_like(q), torch.empty_like(q)
        ptrs = [x.data_ptr() for x in (q, k, v, pos, u, vb, lens)]

        def infer():
            _lib.check(lib.ob_relattn_infer(*ptrs, B, 1, T, H, d, ctx.data_ptr(), s), "infer")

        def fwd():
            _lib.check(lib.ob_relattn_fwd(*ptrs, B, 1, T, H, d, 0.0, None, 0, None, None,
                                          ctx_f.data_ptr(), s), "fwd")

        def core():
            return torch_core(q, k, v, pos, u, vb, mask, H)

        sides = {"infer": infer, "torch": core}
        if T <= 512:
            sides["fwd"] = fwd
        with torch.no_grad():
            reps = {}
            for name, fn in sides.items():  # warm, then size the window from a short timing
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                reps[name] = max(3, min(4000, int(a.window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1))
            diff = (ctx - core()).abs().max().item()
            us = {name: [] for name in sides}
            for name, fn in sides.items():  # one window a side that is not counted
                timed(fn, reps[name])
            for _ in range(a.rounds):
                for name, fn in sides.items():
                    us[name].append(timed(fn, reps[name]))
        med = {name: statistics.median(x) for name, x in us.items()}
        pairs = B * H * T * T
        rec = {"B": B, "T": T, "H": H, "d": d, "key_chunk": kc,
               "infer_us": round(med["infer"], 2), "torch_us": round(med["torch"], 2),
               "torch_over_infer": round(med["torch"] / med["infer"], 2),
               "infer_ps_per_pair": round(med["infer"] * 1e6 / pairs, 3),
               "infer_min_max_us": [round(min(us["infer"]), 2), round(max(us["infer"]), 2)],
               "torch_min_max_us": [round(min(us["torch"]), 2), round(max(us["torch"]), 2)],
               "max_abs_diff_vs_torch": diff, "reps": reps, "rounds": a.rounds}
        if "fwd" in med:
            rec.update(fwd_us=round(med["fwd"], 2),
                       infer_over_fwd=round(med["infer"] / med["fwd"], 2),
                       fwd_ps_per_pair=round(med["fwd"] * 1e6 / pairs, 3),
                       fwd_min_max_us=[round(min(us["fwd"]), 2), round(max(us["fwd"]), 2)])
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del q, k, v, pos, mask, ctx, ctx_f


if __name__ == "__main__":
    main()
