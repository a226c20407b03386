"""GPU: ob_frontend_fwd (csrc/frontend.hip) through onebit_asr.frontend against the fp64
restatement in tests/frontend_ref.py, on a ragged batch whose lengths sit on every frame-count
edge (399 / 400 / 559 / 560 samples), below and above the time-mask width (101 and 204 frames)
and off the kernel's 16 frames per block.

Accuracy bar (log-mel against fp64): max(4 * e32, 2 ulp of the largest |fbank|), where e32 is the
error of the same arithmetic in torch fp32 on the host (``fbank_ref32``) on the same inputs; the
factor 4 covers another butterfly and summation order at the same precision. Measured on MI355X
for this batch (n_mels 80 / 23): e32 2.7e-4 / 1.9e-5 (set by the lowest filter's
weakest frames, whose energy is ~1e-7 of the frame's), the kernel 1.3e-4 / 1.2e-5.
"""
import numpy as np
import pytest
import torch

import frontend_ref as fr

pytestmark = pytest.mark.gpu

LENS = [399, 400, 559, 560, 1680, 1700, 16400, 33000]
FRAMES = [0, 1, 1, 2, 9, 9, 101, 204]
N_MAX = 33000
T = 204
PAD = 24  # floats of NaN on each side of a row


@pytest.fixture(scope="module")
def waves():
    w = fr.make_wave(LENS, N_MAX, seed=0)
    assert [fr.num_frames(n) for n in LENS] == FRAMES and fr.num_frames(N_MAX) == T
    return w


@pytest.fixture(scope="module")
def refs(waves):
    """Per n_mels: (fp64 feats [B, T, n_mels], e32). Computed once, never modified."""
    out = {}
    for n_mels in (80, 23):
        feats, lens = fr.frontend(waves, LENS, n_mels=n_mels)
        assert lens.tolist() == FRAMES
        e32 = 0.0
        for b, n in enumerate(LENS):
            if FRAMES[b]:
                r32 = fr.fbank_ref32(waves[b, :n], n_mels).double().numpy()
                e32 = max(e32, float(np.abs(r32 - feats[b, :FRAMES[b]]).max()))
        feats.setflags(write=False)
        out[n_mels] = (feats, e32)
    return out


def _guarded(waves, gpu):
    """The batch as a view with wave_stride > n_max inside a NaN buffer; the samples past each
    utterance's length are NaN too, so any read outside an utterance shows in the output."""
    buf = torch.full((len(LENS), N_MAX + 2 * PAD), float("nan"), dtype=torch.float32)
    for b, n in enumerate(LENS):
        buf[b, PAD:PAD + n] = torch.from_numpy(waves[b, :n])
    buf = buf.to(gpu)
    view = buf[:, PAD:PAD + N_MAX]
    assert view.stride(0) == N_MAX + 2 * PAD and not view.is_contiguous()
    return view


def _bar(ref, e32):
    ulp = float(np.spacing(np.float32(np.abs(ref).max())))
    return max(4.0 * e32, 2.0 * ulp)


def _cmvn(n_mels):
    g = np.random.default_rng(5)
    mean = g.uniform(-3.0, 3.0, n_mels).astype(np.float32)
    std = g.uniform(0.5, 2.0, n_mels).astype(np.float32)
    return mean, std


STARTS = [[0, 52, 0, 0], [5, 30, 0, 0], [0, 0, 0, 0], [52, 52, 0, 0], [10, 40, 0, 0],
          [3, 27, 0, 0], [0, 52, 0, 0], [7, 44, 3, 103]]


@pytest.mark.parametrize("n_mels", [80, 23])
def test_ragged_batch_matches_fp64(gpu, waves, refs, n_mels):
    from onebit_asr.frontend import fbank_batch

    ref, e32 = refs[n_mels]
    feats, lens = fbank_batch(_guarded(waves, gpu), torch.tensor(LENS, device=gpu), n_mels=n_mels)
    assert feats.shape == (len(LENS), T, n_mels) and feats.dtype == torch.float32
    assert lens.dtype == torch.int64 and lens.tolist() == FRAMES
    got = feats.cpu().numpy()
    assert np.isfinite(got).all()  # no NaN: nothing outside an utterance was read
    for b, m in enumerate(FRAMES):
        assert not got[b, m:].any(), f"pad rows of utterance {b}"
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bar = _bar(ref, e32)
    print(f"n_mels={n_mels}: e32={e32:.3e} gpu_err={err:.3e} bar={bar:.3e} "
          f"max|fbank|={np.abs(ref).max():.3f}")
    # the inputs keep every energy above the log floor (-15.94), here by a factor of e^2 at least
    assert ref[ref != 0].min() > np.log(1.1920929e-07) + 2.0
    assert err <= bar, (err, bar, e32)


def test_lengths_above_n_max_are_clamped(gpu, waves, refs):
    from onebit_asr.frontend import fbank_batch

    n_max = 1700
    buf = torch.full((3, n_max + 2 * PAD), float("nan"), dtype=torch.float32)
    buf[:, PAD:PAD + n_max] = torch.from_numpy(waves[:3, :n_max])
    view = buf.to(gpu)[:, PAD:PAD + n_max]
    feats, lens = fbank_batch(view, torch.tensor([1 << 40, -7, 1701], device=gpu))
    assert lens.tolist() == [9, 0, 9]
    got = feats.cpu().numpy()
    assert np.isfinite(got).all() and not got[1].any()
    want, _ = fr.frontend(waves[:3, :n_max], [n_max, 0, n_max])
    assert np.abs(got - want).max() <= _bar(want, refs[80][1])


@pytest.mark.parametrize("n_mels", [80, 23])
def test_cmvn_matches_fp64(gpu, waves, refs, n_mels):
    from onebit_asr.frontend import FrontEnd

    plain, e32 = refs[n_mels]
    mean, std = _cmvn(n_mels)
    ref, _ = fr.frontend(waves, LENS, n_mels=n_mels, cmvn_mean=mean, cmvn_std=std)
    fe = FrontEnd({"mean": torch.from_numpy(mean), "std": torch.from_numpy(std)},
                  n_mels=n_mels).to(gpu).eval()
    out = fe(_guarded(waves, gpu), torch.tensor(LENS, device=gpu))
    assert out["feat_lens"].tolist() == FRAMES
    got = out["feats"].cpu().numpy()
    for b, m in enumerate(FRAMES):
        assert not got[b, m:].any()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bar = _bar(plain, e32) / float(std.min())  # the log-mel bar over min(std)
    print(f"cmvn n_mels={n_mels}: gpu_err={err:.3e} bar={bar:.3e}")
    assert err <= bar, (err, bar)


def test_zero_waveform_is_the_log_floor(gpu):
    from onebit_asr.frontend import fbank_batch

    lens = [1700, 400, 3000]
    feats, fl = fbank_batch(torch.zeros(3, 3000, device=gpu), torch.tensor(lens, device=gpu))
    assert fl.tolist() == [9, 1, 17]
    got = feats.cpu().numpy()
    want = np.log(np.float32(1.1920929e-07), dtype=np.float32)
    for b, m in enumerate(fl.tolist()):
        assert np.abs(got[b, :m] - want).max() <= np.spacing(np.abs(want))
        assert not got[b, m:].any()


def test_spec_augment_masks(gpu, waves):
    from onebit_asr.frontend import FrontEnd

    mean, std = _cmvn(80)
    fe = FrontEnd(torch.from_numpy(mean), torch.from_numpy(std), spec_augment={}).to(gpu)
    wave, lens = torch.from_numpy(waves).to(gpu), torch.tensor(LENS, device=gpu)
    starts = torch.tensor(STARTS, dtype=torch.int32, device=gpu)
    plain = fe.eval()(wave, lens, starts)["feats"]  # eval mode: no masks, starts ignored
    assert torch.equal(plain, FrontEnd(torch.from_numpy(mean), torch.from_numpy(std)).to(gpu)(
        wave, lens)["feats"])
    out = fe.train()(wave, lens, starts)
    assert out["feat_lens"].tolist() == FRAMES
    got, plain = out["feats"].cpu().numpy(), plain.cpu().numpy()
    for b, m in enumerate(FRAMES):
        keep = fr.spec_augment(np.ones((m, 80)), STARTS[b], 2, 27, 2, 100).astype(bool)
        if m <= 100:
            assert not keep.any()  # the reference zeroes such an utterance whole
        assert (got[b, :m][~keep] == 0.0).all()
        assert (got[b, :m][keep].view(np.uint32) == plain[b, :m][keep].view(np.uint32)).all()
        assert (plain[b, :m] != 0.0).all() and not got[b, m:].any()
    assert got[6, 100].any() and not got[6, :100].any()      # 101 frames: mask [0, 100)
    assert got[7, 0:3].any() and not got[7, 3:203].any() and got[7, 203].any()
    # drawn starts in training mode: every utterance of at most 100 frames comes out zero
    drawn = fe(wave, lens)["feats"]
    assert not drawn[:6].any() and drawn[7].any()
    assert torch.equal(fe(wave, lens, starts)["feats"], out["feats"])  # reproducible


def test_draw_specaug_starts_stays_in_range(gpu):
    from onebit_asr.frontend import draw_specaug_starts

    m = torch.tensor(FRAMES + [100, 734], device=gpu).repeat(1000)  # 1000 draws per length
    g = torch.Generator(device=gpu).manual_seed(1)
    s = draw_specaug_starts(m, generator=g)
    assert s.shape == (m.numel(), 4) and s.dtype == torch.int32 and s.is_cuda
    hi_t = torch.tensor([fr.start_range(int(v), 100) for v in m.tolist()], device=gpu)
    assert (s >= 0).all() and (s[:, :2] < fr.start_range(80, 27)).all()
    assert (s[:, 2:] < hi_t[:, None]).all()
    per_len = s[:, 2:].reshape(1000, -1, 2).amax(dim=(0, 2)).tolist()
    assert per_len[:7] == [0] * 7 and per_len[8] == 0  # m <= 101: the only start is 0
    assert 95 <= per_len[7] <= 103 and 600 <= per_len[9] <= 633
    assert s[:, :2].max().item() == 52 and s[:, :2].min().item() == 0
    s23 = draw_specaug_starts(m, generator=g, n_mels=23)  # 23 bins < 27: width 23, start 0
    assert not s23[:, :2].any()
    g.manual_seed(1)
    assert torch.equal(draw_specaug_starts(m, generator=g), s)


def test_graph_capture_replays_bitwise(gpu, waves):
    from onebit_asr.frontend import FrontEnd

    mean, std = _cmvn(80)
    fe = FrontEnd(torch.from_numpy(mean), torch.from_numpy(std), spec_augment={}).to(gpu).train()
    wave, lens = torch.from_numpy(waves).to(gpu), torch.tensor(LENS, device=gpu)
    starts = torch.tensor(STARTS, dtype=torch.int32, device=gpu)
    eager = fe(wave, lens, starts)
    again = fe(wave, lens, starts)
    assert torch.equal(eager["feats"], again["feats"])
    assert torch.equal(eager["feat_lens"], again["feat_lens"])
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fe(wave, lens, starts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe(wave, lens, starts)
    graph.replay()
    assert torch.equal(out["feats"], eager["feats"])
    assert torch.equal(out["feat_lens"], eager["feat_lens"])
    # other inputs through the same graph
    wave.copy_(torch.from_numpy(fr.make_wave(LENS, N_MAX, seed=9)).to(gpu))
    lens.copy_(torch.tensor(LENS[::-1], device=gpu))
    graph.replay()
    want = fe(wave, lens, starts)
    assert torch.equal(out["feats"], want["feats"])
    assert out["feat_lens"].tolist() == FRAMES[::-1]


def test_graphed_inference_with_frontend(gpu):
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1
    from onebit_asr.frontend import FrontEnd
    from onebit_asr.infer import GraphedInference

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to(gpu).eval()
    mean, std = _cmvn(80)
    fe = FrontEnd(torch.from_numpy(mean), torch.from_numpy(std), spec_augment={}).to(gpu)
    n_max, lens = 16400, [16400, 9000]
    tokens = torch.randint(4, 5004, (2, 7), device=gpu)
    batches = []
    for seed in (0, 1):
        w = torch.from_numpy(fr.make_wave(lens, n_max, seed=seed)).to(gpu)
        batches.append({"wave": w, "wave_lens": torch.tensor(lens, device=gpu), "tokens": tokens,
                        "token_lens": torch.tensor([7, 5], device=gpu)})
    gi = GraphedInference(model, precision=2, frontend=fe)
    assert not fe.training  # inference: no SpecAugment
    got = [tuple(t.clone() for t in gi.run(b)) for b in (batches[0], batches[1], batches[0])]
    plain = GraphedInference(model, precision=2)
    for b, (out, cnt, logits) in zip((batches[0], batches[1], batches[0]), got):
        feats = fe(b["wave"], b["wave_lens"])
        assert feats["feat_lens"].tolist() == [101, 54]
        ref = plain.run({**feats, "tokens": b["tokens"], "token_lens": b["token_lens"]})
        assert torch.equal(logits, ref[2])
        assert torch.equal(out, ref[0]) and torch.equal(cnt, ref[1])
        assert cnt.min().item() >= 0 and logits.isfinite().all()
    assert not torch.equal(got[0][2], got[1][2]) and torch.equal(got[0][2], got[2][2])
