#!/usr/bin/env python3
"""Feature front end timing at the training batch (32 x 160 400 samples = 1000 frames each,
seeded noise + tones): ``FrontEnd`` plain (fbank only) and with CMVN + SpecAugment, HIP events
around each call on the launch stream after warm-up, the median and the spread over --reps
calls; and the host path the kernel replaces, ``fbank_ref32`` (tests/frontend_ref.py: the
reference's torchaudio arithmetic in torch fp32) plus CMVN per utterance on --threads CPU
threads (one utterance per task). ``fbank_graph`` is the plain call replayed from a captured HIP
graph (no Python between the events). The byte floor is (samples read + features written) * 4 B
over 8 TB/s, the HBM rate DESIGN.md uses. Prints one JSON line.
Usage: python tools/frontend_bench.py [--reps 30] [--batch 32] [--samples 160400] [--threads 16]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tests")]

import torch  # noqa: E402

from frontend_ref import fbank_ref32, make_wave  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.frontend import FrontEnd, fbank_num_frames  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


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


def host_path(wave, mean, std, threads, reps):
    """Seconds for the whole batch: one utterance per task on a pool of ``threads`` threads with
    one intra-op thread each, as the reference's DataLoader workers split it (torch releases
    the GIL inside its ops). Best of ``reps``."""
    from concurrent.futures import ThreadPoolExecutor

    torch.set_num_threads(1)

    def one(b):
        return (fbank_ref32(wave[b]) - mean) / std

    best = float("inf")
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(reps + 1):  # the first pass warms the FFT plans up
            t0 = time.perf_counter()
            list(pool.map(one, range(wave.shape[0])))
            best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=160400)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.batch, args.samples
    frames = fbank_num_frames(n)
    cpu_wave = torch.from_numpy(make_wave([n] * B, n, seed=0))
    wave = cpu_wave.to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    g = torch.Generator().manual_seed(0)
    mean = torch.randn(80, generator=g)
    std = torch.rand(80, generator=g) * 1.5 + 0.5
    plain = FrontEnd().to(dev).eval()
    full = FrontEnd(mean, std, spec_augment={}).to(dev).train()
    starts = torch.tensor([[5, 40, 100, 600]] * B, dtype=torch.int32, device=dev)
    res = {"fbank": timed(lambda: plain(wave, lens), args.reps, args.warmup),
           "fbank_cmvn_specaug": timed(lambda: full(wave, lens, starts), args.reps, args.warmup),
           "fbank_cmvn_specaug_drawn": timed(lambda: full(wave, lens), args.reps, args.warmup)}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = plain(wave, lens)
    res["fbank_graph"] = timed(graph.replay, args.reps, args.warmup)
    assert torch.equal(held["feats"], plain(wave, lens)["feats"])
    floor_us = (B * n + B * frames * 80) * 4 / HBM_BYTES_PER_S * 1e6
    for v in res.values():
        v["frames_per_s"] = round(B * frames / (v["median_us"] * 1e-6))
        v["x_byte_floor"] = round(v["median_us"] / floor_us, 1)
    host_s = host_path(cpu_wave, mean, std, args.threads, args.host_reps)
    print(json.dumps({"tool": "frontend_bench", "device": torch.cuda.get_device_name(0),
                      "B": B, "samples": n, "frames": frames, "reps": args.reps,
                      "byte_floor_us": round(floor_us, 2), **res,
                      "host_ref32_cmvn": {"threads": args.threads, "ms": round(host_s * 1e3, 1),
                                          "frames_per_s": round(B * frames / host_s)},
                      "host_over_device": round(host_s * 1e6 / res["fbank"]["median_us"], 1),
                      "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
