"""CPU: the fp64 restatement of the feature front end (tests/frontend_ref.py) against
hand-derived answers, and the host half of the library (frame count, table, argument checks).
No GPU is needed: nothing here launches."""
import math

import numpy as np
import pytest
import torch

import frontend_ref as fr

LOG_FLOOR = math.log(float(np.float32(1.1920929e-07)))


def _lib():
    from onebit_asr import _lib as L

    return L, L.load()


@pytest.mark.parametrize("n,m", [(0, 0), (399, 0), (400, 1), (559, 1), (560, 2), (117760, 734)])
def test_frame_counts(n, m):
    assert fr.num_frames(n) == m
    assert fr.frames_of(np.zeros(n)).shape == (m, 400)
    _, lib = _lib()
    assert lib.ob_fbank_num_frames(n) == m
    from onebit_asr.frontend import fbank_num_frames

    assert fbank_num_frames(n) == m


def test_mel_scale():
    assert abs(float(fr.mel(1000.0)) - 1000.0) <= 0.02
    assert float(fr.mel(0.0)) == 0.0


@pytest.mark.parametrize("n_mels", [80, 23])
def test_mel_bank_structure(n_mels):
    bank = fr.mel_bank(n_mels)
    assert bank.shape == (n_mels, 257)
    assert not bank[:, 0].any() and not bank[:, 256].any()
    assert ((bank > 0).sum(axis=0) <= 2).all()
    assert (bank >= 0).all() and bank.max() <= 1.0
    lo, hi = float(fr.mel(20.0)), float(fr.mel(8000.0))
    d = (hi - lo) / (n_mels + 1)
    mk = fr.mel(np.arange(256) * 31.25)
    inside = (mk >= lo + d) & (mk <= lo + n_mels * d)  # first .. last filter centre
    assert inside.sum() > 200
    assert np.abs(bank[:, :256].sum(axis=0)[inside] - 1.0).max() <= 1e-12
    # every filter's non-zero bins are contiguous (what the library's sparse form relies on)
    for f in range(n_mels):
        nz = np.flatnonzero(bank[f])
        assert nz.size == 0 or (np.diff(nz) == 1).all()


def test_constant_waveform_is_the_log_floor():
    v = fr.fbank(np.full(1000, 0.37))
    assert v.shape == (4, 80)
    assert (v == LOG_FLOOR).all()
    feats, lens = fr.frontend(np.full((1, 1000), 0.37, dtype=np.float32), [1000])
    assert lens.tolist() == [4] and (feats == LOG_FLOOR).all()


def test_parseval_and_direct_dft():
    x = fr.make_wave([400], 400, seed=3)[0]
    y = fr.windowed_frames(x)
    p = fr.power_spectrum(y)[0]
    total = p[0] + p[256] + 2.0 * p[1:256].sum()
    want = 512.0 * float((y[0] ** 2).sum())
    assert abs(total - want) <= 1e-12 * want
    j = np.arange(400)
    k = np.arange(257)[:, None]
    direct = (y[0][None, :] * np.exp(-2j * math.pi * k * j[None, :] / 512.0)).sum(axis=1)
    assert np.abs(np.abs(direct) ** 2 - p).max() <= 1e-12 * p.max()


def test_preemphasis_and_window_by_hand():
    out = fr.preemphasis(np.array([[1.0, 2.0, 4.0, -1.0]]))
    assert np.allclose(out, [[0.03, 2.0 - 0.97, 4.0 - 1.94, -1.0 - 3.88]], rtol=0, atol=1e-15)
    assert np.allclose(fr.remove_dc(np.array([[1.0, 2.0, 6.0]])), [[-2.0, -1.0, 3.0]])
    w = fr.povey_window()
    assert w[0] == 0.0 and abs(w[399]) <= 1e-12  # (0.5 - 0.5 cos 0)^0.85
    assert np.allclose(w, w[::-1], rtol=0, atol=1e-12)
    # j = 133: 2 pi 133 / 399 = 2 pi / 3, cos = -1/2, so w = 0.75^0.85
    assert abs(w[133] - 0.75 ** 0.85) <= 1e-14
    assert abs(w[199] - (0.5 - 0.5 * math.cos(2 * math.pi * 199 / 399)) ** 0.85) <= 1e-15
    assert w.argmax() in (199, 200) and w.max() <= 1.0


def test_spec_augment_by_hand():
    v = np.arange(1.0, 1.0 + 6 * 5).reshape(6, 5)  # 6 frames, 5 bins, no zero in it
    out = fr.spec_augment(v, [1, 3, 0, 4], n_fmask=2, fmask_w=2, n_tmask=2, tmask_w=1)
    want = v.copy()
    want[:, 1:3] = 0.0
    want[:, 3:5] = 0.0
    want[0:1] = 0.0
    want[4:5] = 0.0
    assert (out == want).all()
    assert (out[1:4, 0] == v[1:4, 0]).all() and (v != 0).all()  # the input is not touched
    # m <= the time-mask width: the width is m, the only start is 0, everything is zeroed
    assert fr.start_range(6, 100) == 1 and fr.start_range(100, 100) == 1
    out = fr.spec_augment(v, [0, 0, 0, 0], n_fmask=0, fmask_w=27, n_tmask=1, tmask_w=100)
    assert not out.any()
    # the start ranges: [0, size - width), but never empty
    assert fr.start_range(80, 27) == 53 and fr.start_range(101, 100) == 1
    assert fr.start_range(204, 100) == 104 and fr.start_range(20, 27) == 1
    # a mask that starts at the last allowed place ends at the edge
    out = fr.spec_augment(v, [3], n_fmask=1, fmask_w=2, n_tmask=0, tmask_w=0)
    assert (out[:, 3:] == 0).all() and (out[:, :3] == v[:, :3]).all()


def test_frontend_pads_and_clamps():
    wave = fr.make_wave([1700, 399], 1700)
    feats, lens = fr.frontend(wave, [1700, 399], T=12)
    assert lens.tolist() == [9, 0] and feats.shape == (2, 12, 80)
    assert not feats[0, 9:].any() and not feats[1].any() and feats[0, :9].all()
    feats2, lens2 = fr.frontend(wave, [5000, -3], T=12)  # lengths are clamped to [0, n_max]
    assert lens2.tolist() == [9, 0] and (feats2 == feats).all()
    mean, std = np.linspace(-1, 1, 80), np.linspace(0.5, 2, 80)
    featsc, _ = fr.frontend(wave, [1700, 399], T=12, cmvn_mean=mean, cmvn_std=std)
    assert np.allclose(featsc[0, :9], (feats[0, :9] - mean) / std, rtol=0, atol=1e-13)
    assert not featsc[0, 9:].any()


def test_ref32_tracks_the_restatement():
    x = fr.make_wave([1700], 1700, seed=1)[0]
    e32 = np.abs(fr.fbank_ref32(x).double().numpy() - fr.fbank(x)).max()
    assert 0 < e32 <= 1e-4, e32


@pytest.mark.parametrize("n_mels", [80, 23, 1, 128])
def test_table_fill_equals_the_restatement(n_mels):
    from onebit_asr.frontend import frontend_table, unpack_table

    L, lib = _lib()
    table = frontend_table(n_mels)
    assert table.numel() == lib.ob_frontend_table_floats(n_mels) == 400 + 1024 + 3 * n_mels + 512
    window, tw, bank = unpack_table(table, n_mels)
    assert (window.numpy() == fr.povey_window().astype(np.float32)).all()
    assert (tw.numpy() == fr.twiddles().astype(np.float32)).all()
    assert (bank.numpy() == fr.mel_bank(n_mels).astype(np.float32)).all()
    # the descriptors: whole numbers, weights packed filter after filter, tail zero
    desc = table[1424:1424 + 3 * n_mels].reshape(n_mels, 3)
    assert (desc == desc.round()).all()
    used = int(desc[:, 1].sum())
    assert used <= 510 and (desc[:, 0] + desc[:, 1] <= 256).all()
    assert (desc[:, 2] == torch.cumsum(desc[:, 1], 0) - desc[:, 1]).all()
    assert not table[1424 + 3 * n_mels + used:].any()


def test_table_argument_checks():
    _, lib = _lib()
    buf = torch.empty(4000, dtype=torch.float32)
    assert lib.ob_frontend_table_floats(0) == 0 and lib.ob_frontend_table_floats(129) == 0
    assert lib.ob_frontend_table_fill(buf.data_ptr(), 0) == -2
    assert lib.ob_frontend_table_fill(buf.data_ptr(), 129) == -2
    assert lib.ob_frontend_table_fill(None, 80) == -1
    assert lib.ob_frontend_table_fill(buf.data_ptr() + 1, 80) == -5


def test_frontend_fwd_argument_checks_without_gpu():
    """Every check below fails before any HIP call, so it is safe with no device."""
    _, lib = _lib()
    fake = 0x1000  # never dereferenced

    def call(wave=fake, stride=2000, lens=fake, B=2, n_max=2000, table=fake, n_mels=80,
             mean=None, std=None, starts=None, nf=0, wf=0, nt=0, wt=0, feats=fake, T=11,
             flens=fake):
        return lib.ob_frontend_fwd(wave, stride, lens, B, n_max, table, n_mels, mean, std, starts,
                                   nf, wf, nt, wt, feats, T, flens, None)

    assert call(n_mels=0) == -2 and call(n_mels=129) == -2 and call(n_mels=-1) == -2
    assert call(B=-1) == -2 and call(n_max=-1) == -2 and call(T=-1) == -2
    assert call(T=10) == -2  # 2000 samples are 11 frames
    assert call(stride=1999) == -2
    assert call(nf=-1) == -2 and call(wf=-1) == -2 and call(nt=-1) == -2 and call(wt=-1) == -2
    assert call(B=1 << 40, T=1 << 30) == -2  # more blocks than one launch grid holds
    assert call(B=0) == 0  # nothing to launch, also with no pointers
    assert call(B=0, wave=None, lens=None, table=None, feats=None, flens=None) == 0
    for name in ("wave", "lens", "table", "feats", "flens"):
        assert call(**{name: None}) == -1, name
    assert call(mean=fake) == -1 and call(std=fake) == -1  # CMVN: both or neither
    for name in ("wave", "table", "feats"):
        assert call(**{name: fake + 2}) == -5, name
    assert call(mean=fake + 1, std=fake) == -5 and call(starts=fake + 2, nf=1) == -5
    assert call(lens=fake + 4) == -5 and call(flens=fake + 4) == -5


def test_python_surface_on_cpu():
    import onebit_asr
    from onebit_asr.frontend import FrontEnd, draw_specaug_starts, fbank_batch

    assert onebit_asr.FrontEnd is FrontEnd and onebit_asr.fbank_batch is fbank_batch
    assert onebit_asr.draw_specaug_starts is draw_specaug_starts
    wave, lens = torch.zeros(2, 800), torch.tensor([800, 400])
    with pytest.raises(RuntimeError, match=r"runs on the HIP library \(no CPU fallback\)"):
        fbank_batch(wave, lens)
    fe = FrontEnd(cmvn_mean={"mean": torch.zeros(80), "std": torch.ones(80)}, spec_augment={})
    assert fe.cmvn_std.shape == (80,) and fe.spec_augment["time_mask_param"] == 100
    assert set(fe.state_dict()) == {"cmvn_mean", "cmvn_std"}
    with pytest.raises(RuntimeError, match=r"runs on the HIP library \(no CPU fallback\)"):
        fe(wave, lens)
    with pytest.raises(ValueError):
        FrontEnd(cmvn_mean=torch.zeros(80))
    with pytest.raises(ValueError):
        FrontEnd(n_mels=129)
    # the start helper is plain torch: on the CPU it can be checked against the ranges
    m = torch.tensor([0, 1, 100, 101, 204, 734])
    g = torch.Generator().manual_seed(0)
    hi_t = torch.tensor([fr.start_range(int(v), 100) for v in m])
    seen = torch.zeros(6, dtype=torch.long)
    for _ in range(200):
        s = draw_specaug_starts(m, generator=g)
        assert s.shape == (6, 4) and s.dtype == torch.int32
        assert (s >= 0).all() and (s[:, :2] < 53).all() and (s[:, 2:] < hi_t[:, None]).all()
        seen = torch.maximum(seen, s[:, 2:].max(dim=1).values.long())
    assert seen[:4].tolist() == [0, 0, 0, 0] and seen[4] > 90 and seen[5] > 600
