#!/usr/bin/env python3
"""Decode timing at the inference batch (B = 256, T = 249, V = 5004, ragged lens, seeded
CTC-like logits): greedy decode (ob_ctc_greedy_decode), and the two launches of the beam search
on their own (ob_ctc_beam_search_stage: 1 = per-frame log-softmax + top-k, 2 = the serial
search) and together. HIP events around each call on the launch stream, after warm-up of every
shape; the median and the spread over --reps calls. Prints one JSON line.
Usage: python tools/decode_bench.py [--reps 30] [--beam 10] [--top-k 20]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd")]

import torch  # noqa: E402

from onebit_asr import _lib  # noqa: E402
from onebit_asr.infer import ctc_beam_search_batch_device, ctc_greedy_decode_batch  # noqa: E402


def ctc_like_logits(B, T, V, blank, seed, dev):
    """Unit normal noise plus a +3 peak per frame: blank half the time, else one of 6 tokens."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    toks = torch.randperm(V - 4, generator=g)[:6] + 4
    peak = torch.where(torch.rand(B, T, generator=g) < 0.5, torch.tensor(blank),
                       toks[torch.randint(0, 6, (B, T), generator=g)])
    x.scatter_add_(2, peak.unsqueeze(-1), torch.full((B, T, 1), 3.0))
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    return x.to(dev), lens.to(dev)


def timed(fn, reps, warmup):
    """us per call: (median, min, max) of per-call event pairs."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(st)
        fn()
        e1.record(st)
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1),
            "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--blank", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V = args.batch, args.frames, args.vocab
    x, lens = ctc_like_logits(B, T, V, args.blank, 0, dev)
    need = lib.ob_ctc_beam_search_workspace(B, T, V, args.beam, args.top_k)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    out = torch.empty(B, T, dtype=torch.int32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)

    def stage(k):
        def run():
            _lib.check(lib.ob_ctc_beam_search_stage(
                x.data_ptr(), lens.data_ptr(), B, T, V, args.blank, args.beam, args.top_k, k,
                ws.data_ptr(), need, out.data_ptr(), cnt.data_ptr(), score.data_ptr(),
                _lib.stream_of(x)), "ob_ctc_beam_search_stage")
        return run

    res = {"greedy": timed(lambda: ctc_greedy_decode_batch(x, lens, args.blank), args.reps,
                           args.warmup),
           "beam_frames": timed(stage(1), args.reps, args.warmup),
           "beam_search": timed(stage(2), args.reps, args.warmup),
           "beam_both": timed(stage(0), args.reps, args.warmup)}
    frames = int(lens.max().item())
    res["beam_search_us_per_frame_longest"] = round(res["beam_search"]["median_us"] / frames, 2)
    # the Python entry (allocations included) gives what an eval loop sees, and the same result
    o2, c2, s2 = ctc_beam_search_batch_device(x, lens, args.beam, args.blank, args.top_k)
    same = bool(torch.equal(o2, out) and torch.equal(c2, cnt) and torch.equal(s2, score))
    g_out, g_cnt = ctc_greedy_decode_batch(x, lens, args.blank)
    differ = int((g_out != o2).any(dim=1).sum().item())
    print(json.dumps({"tool": "decode_bench", "device": torch.cuda.get_device_name(0),
                      "B": B, "T": T, "V": V, "beam": args.beam, "top_k": args.top_k,
                      "frames_total": int(lens.sum().item()), "workspace_bytes": need,
                      "reps": args.reps, **res, "python_entry_matches": same,
                      "utterances_where_beam_differs_from_greedy": differ,
                      "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
