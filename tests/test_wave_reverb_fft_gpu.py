"""The transform route of the reverberation on the device (-m gpu): ``WaveAugment(reverb="fft")`` (deeplip_amd/augment.py, DESIGN.md
section 4i) against the fp64 definition at the overlap-save block's edges; against the direct route; the exact cases; padding never
read; each row as if alone; inside a recorded plan; in front of the front-end and an encoder; in train_audio's from-waves mode.

Geometry, with P = DLIP_OLS_BLOCK: one batch padded to S = 3P + 3 samples whose rows hold n = 3P + 3, 2P, P + 1, P, P - 1 and 1
samples; room responses of 1, 2, P, P + 1, 2P + 5, DLIP_FIR_MAX_TAPS + 1 and 3P + 1 taps (1 .. ceil(8193 / P) partitions in one bank) with the
direct path at tap 0, mid-way or at the last tap.  Bars: the project's output bar rel_err < 2e-5 per row against fp64 (as the direct
route), twice that between the routes, the front-end's 1e-4 behind it.

Measured on an MI355X (EXPERIMENTS.md R15.1): worst rel_err against fp64 5.5e-7 with keep_power off and 5.2e-7 with it on; the
single-shot fp32 torch.fft yardstick on the CPU 3.7e-7 on the same rows; the two routes differ by at most 3.0e-6."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err
from deeplip_amd import _lib, weightgen as wg
from test_models_gpu import DEV, load, tdnn_opts
from test_wave_augment_gpu import SMALL, _params, ref_reverb, ref_row

pytestmark = pytest.mark.gpu

P, T = _lib.DLIP_OLS_BLOCK, _lib.DLIP_FIR_TILE
S = 3 * P + 3
LENS = (3 * P + 3, 2 * P, P + 1, P, P - 1, 1)
B = len(LENS)
RIR_PEAKS = ((1, 0), (2, 1), (P, P // 2), (P + 1, 0), (2 * P + 5, 2 * P + 4), (_lib.DLIP_FIR_MAX_TAPS + 1, 7), (3 * P + 1, P))
NR = len(RIR_PEAKS)
SHORT = [i for i, (n, _) in enumerate(RIR_PEAKS) if n <= _lib.DLIP_FIR_MAX_TAPS]          # the responses the direct route takes
BANK = 2 * S
BAR = 2e-5                                                                                # README, "project bars"


@functools.lru_cache(maxsize=None)
def _signals():
    t = np.arange(S) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (210 + 140 * b) * t) + 0.05 * wg.gen(f"wf.sig{b}", (S,)) for b in range(B)]).astype(np.float32)
    sig.setflags(write=False)
    return sig


@functools.lru_cache(maxsize=None)
def _rirs():
    out = []
    for i, (n, p) in enumerate(RIR_PEAKS):
        h = 0.1 * wg.gen(f"wf.rir{i}", (n,))
        h[p] = 1.0 if i % 2 == 0 else -1.0
        h = h.astype(np.float32)
        h.setflags(write=False)
        out.append(h)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _bank():
    b = (0.2 * wg.gen("wf.bank", (BANK,))).astype(np.float32)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _want(b, r, keep_power):
    """The definition in fp64 for row b through response r (computed once, shared by the tests)."""
    want = ref_row(_signals()[b], LENS[b], rir=(_rirs()[r], RIR_PEAKS[r][1]), keep_power=keep_power, stage32=False)
    want.setflags(write=False)
    return want


def _batch(fill=0.0, lens=LENS):
    x = np.full((len(lens), S), fill, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = _signals()[b, :n]
    return torch.from_numpy(x).to(DEV)


def _lens_dev(vals=LENS):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def _aug(**kw):
    from deeplip_amd.augment import WaveAugment
    kw.setdefault("reverb", "fft")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                            # no response of these tests is truncated
        return WaveAugment(**kw)


def _fft32(x, h, d):
    """The yardstick: one single-shot fp32 rfft / irfft convolution on the CPU."""
    n = x.size
    N = 1 << int(np.ceil(np.log2(n + h.size)))
    y = torch.fft.irfft(torch.fft.rfft(torch.from_numpy(x.copy()), n=N) * torch.fft.rfft(torch.from_numpy(h.copy()), n=N), n=N)
    assert y.dtype == torch.float32
    return y.numpy()[d:d + n]


# --------------------------------------------------------------------------------------------------- 1. against the definition
@pytest.mark.parametrize("keep_power", [False, True])
def test_fft_route_against_fp64(keep_power):
    aug = _aug(rirs=_rirs(), p_reverb=1.0, keep_power=keep_power)
    assert aug.truncated == [] and aug.rir_len.tolist() == [n for n, _ in RIR_PEAKS] and aug.rir_peak.tolist() == [p for _, p in RIR_PEAKS]
    assert len({(n + P - 1) // P for n, _ in RIR_PEAKS}) >= 4                              # differing partition counts in one bank
    assert sum(n > min(LENS[:-1]) for n, _ in RIR_PEAKS) >= 3                              # responses longer than the shortest rows
    x = _batch()
    sig = _signals()
    worst = worst32 = 0.0
    for shift in range(NR):                                                                # every row meets every response
        ridx = [(b + shift) % NR for b in range(B)]
        y = aug(x, list(LENS), params=_params(ridx=ridx)).cpu().numpy()
        for b, n in enumerate(LENS):
            h, d = _rirs()[ridx[b]], RIR_PEAKS[ridx[b]][1]
            e = rel_err(y[b], _want(b, ridx[b], keep_power))
            # the same sums through a single-shot fp32 transform: the bar measures the kernel, not the conditioning of the data
            e32 = rel_err(_fft32(sig[b, :n], h, d), ref_reverb(sig[b, :n], h, d, False))
            worst, worst32 = max(worst, e), max(worst32, e32)
            print(f"keep_power {keep_power} row {b} (n {n}) response {ridx[b]} ({h.size} taps, d {d}): rel_err {e:.3e}, torch.fft f32 {e32:.3e}")
            assert e32 < BAR / 4, (b, ridx[b])
            assert e < BAR, (b, ridx[b])
            assert not y[b, n:].any()
    print(f"worst rel_err {worst:.3e} (single-shot fp32 torch.fft on the CPU: {worst32:.3e})")


# ------------------------------------------------------------------------------------------------------- 2. both routes agree
@pytest.mark.parametrize("keep_power", [False, True])
def test_both_routes_agree(keep_power):
    rirs = [_rirs()[i] for i in SHORT]
    assert len(rirs) == NR - 1
    fft = _aug(rirs=rirs, p_reverb=1.0, keep_power=keep_power)
    fir = _aug(rirs=rirs, p_reverb=1.0, keep_power=keep_power, reverb="fir")
    x = _batch()
    worst = 0.0
    for shift in range(len(rirs)):
        p = _params(ridx=[(b + shift) % len(rirs) for b in range(B)])
        ya, yb = fft(x, list(LENS), params=p).cpu().numpy(), fir(x, list(LENS), params=p).cpu().numpy()
        for b, n in enumerate(LENS):
            e = rel_err(ya[b], yb[b].astype(np.float64))
            worst = max(worst, e)
            assert e < 2 * BAR, (b, shift)                                                 # each is within the bar of fp64
            assert not ya[b, n:].any()
    print(f"keep_power {keep_power}: the routes differ by at most {worst:.3e}")


# --------------------------------------------------------------------------------------------------------------- 3. exact cases
def test_exact_cases():
    x = _batch()
    x[3] = 0                                                                               # an all-zero row
    clean = x.clone()
    for b, n in enumerate(LENS):
        clean[b, n:] = 0
    for keep_power in (False, True):
        aug = _aug(rirs=_rirs(), p_reverb=0.5, keep_power=keep_power)
        ridx = [-1, 5, -1, 4, -1, -7]
        y = aug(x, list(LENS), params=_params(ridx=ridx))
        for b in (0, 2, 4, 5):
            assert torch.equal(y[b], clean[b]), b                                          # pass-through rows: bit for bit, zero tail
        assert not torch.equal(y[1], clean[1])
        assert not y[3].any() and torch.isfinite(y).all()                                  # zeros in, zeros out; the gain divides by nothing
        # the row of one sample: h[d] x[0] (keep_power: its magnitude restored, the sign of h[d] kept)
        for r, (_, d) in enumerate(RIR_PEAKS):
            got = aug(x, list(LENS), params=_params(ridx=[r] * B))[5].cpu().numpy()
            hd, x0 = float(_rirs()[r][d]), float(_signals()[5, 0])
            want = np.sign(hd) * x0 if keep_power else hd * x0
            assert abs(got[0] - want) < BAR * abs(want) and not got[1:].any(), (keep_power, r)


# ----------------------------------------------------------------------------------------------------- 4. padding is never read
def test_padding_is_never_read_and_the_tail_is_zero(monkeypatch):
    """NaN behind the rows and NaN in every buffer the wrapper takes (the input-spectra workspace among them): the zero-padded
    run's output bit for bit, zeros at t >= n.  Device lengths outside [1, S] are clamped."""
    from deeplip_amd import ops
    real_empty = ops._empty

    def nan_empty(shape, device, dtype=torch.float32):
        return real_empty(shape, device, dtype).fill_(float("nan"))
    for keep_power in (False, True):
        aug = _aug(rirs=_rirs(), p_reverb=1.0, keep_power=keep_power)
        p = _params(ridx=[6, 5, 4, 3, 2, 1])
        want = aug(_batch(0.0), _lens_dev(), params=p)
        monkeypatch.setattr(ops, "_empty", nan_empty)
        outs = [aug(_batch(fill), _lens_dev(), params=p) for fill in (1e30, float("nan"))]
        monkeypatch.setattr(ops, "_empty", real_empty)
        for y in outs:
            assert torch.isfinite(y).all() and torch.equal(y, want)
            for b, n in enumerate(LENS):
                assert not y[b, n:].any() and y[b, :n].any()
    clamped = [S, LENS[1], 1, LENS[3], 1, S]
    xb = _batch(lens=clamped)
    got = aug(xb, _lens_dev([S + 5, LENS[1], 0, LENS[3], -3, 10 ** 6]), params=p)
    assert torch.equal(got, aug(xb, clamped, params=p))


# ----------------------------------------------------------------------------------------------------- 5. each row as if alone
def test_each_row_equals_the_row_alone():
    aug = _aug(rirs=_rirs(), p_reverb=1.0)
    x = _batch(float("nan"))
    for ridx in ([6, 5, 4, 3, 2, 1], [5, 6, 0, 4, 5, 6]):
        y = aug(x, _lens_dev(), params=_params(ridx=ridx))
        for b, n in enumerate(LENS):
            row = x[b:b + 1].contiguous()
            one = aug(row, [n], params=_params(ridx=ridx[b:b + 1]))                        # B = 1, the batch's S
            assert torch.equal(y[b:b + 1], one), b
            trimmed = aug(x[b:b + 1, :n].contiguous(), params=_params(ridx=ridx[b:b + 1]))  # S trimmed to the row's own length
            assert trimmed.shape == (1, n) and torch.equal(y[b:b + 1, :n], trimmed), b
            r = ridx[b]
            own = _aug(rirs=[_rirs()[r]], rir_peaks=[RIR_PEAKS[r][1]], p_reverb=1.0)      # the bank reduced to the row's response
            assert own.rir.shape == (1, RIR_PEAKS[r][0])
            assert torch.equal(y[b:b + 1], own(row, [n], params=_params(ridx=[0]))), b
            assert rel_err(y[b].cpu().numpy(), _want(b, r, True)) < BAR, b


# ------------------------------------------------------------------------------------------------------------------ 6. recorded
def test_a_recorded_plan_follows_new_params_and_lengths():
    from deeplip_amd.plan import StepPlan
    aug = _aug(noise=_bank(), rirs=_rirs(), p_reverb=1.0, normalize=True)

    def step(wave, lens, snr, start, ridx):
        return aug(wave, lens, params={"snr_db": snr, "noise_start": start, "rir_idx": ridx})

    def inputs(fill, lens, snr, start, ridx):
        p = _params(snr=snr, start=start, ridx=ridx)
        return (_batch(fill, lens), _lens_dev(lens)) + tuple(torch.from_numpy(p[k]).to(DEV) for k in ("snr_db", "noise_start", "rir_idx"))

    ins0 = inputs(0.0, LENS, (-5.0, 0.0, 20.0, 9999.0, -5.0, 20.0), (BANK - LENS[0], 17, 3, 5, 0, BANK - 1), [0, 1, 2, 3, 4, 5])
    plan = StepPlan(step, *ins0)
    first = plan.run().clone()
    torch.cuda.synchronize()
    assert torch.equal(first, step(*ins0))
    lens1 = (P, 1, 3 * P + 3, 77, 2 * P - 1, P + 9)
    ins1 = inputs(7.0, lens1, (9999.0, 3.0, 10.0, 0.0, 9999.0, -5.0), (0, 9, 1, 2 * P, 0, 100), [6, -1, 5, 2, -1, 4])
    got = plan(*ins1).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, step(*ins1)) and not torch.equal(got, first)
    print(f"launches in the plan: {plan.launches}")
    assert plan.launches == 8               # reverb 4 (input spectra, accumulate + invert, keep_power 2), noise 2, normalise 2
    plan.close()


# ----------------------------------------------------------------------------------------------------------------- 7. the chain
def test_the_chain_into_frontend_and_encoder():
    from deeplip_amd.frontend import AudioFrontend
    from models.audio_models.tdnn import SpeakerEmbNet
    net, _ = load(SpeakerEmbNet(tdnn_opts()), "wf.chain.")
    fe = AudioFrontend("mfcc")
    lens = [400 + 39 * 160, 6000, 5000, 4100]                                             # 40, 36, 30, 25 frames
    Sp = lens[0]
    t = np.arange(Sp) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (180 + 90 * b) * t) + 0.05 * wg.gen(f"wf.chain.{b}", (Sp,)) for b in range(4)]).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0
    pick = (5, 6)                                                                          # 8193 and 3P + 1 taps
    rirs, bank = [_rirs()[i] for i in pick], (0.2 * wg.gen("wf.chain.bank", (8000,))).astype(np.float32)
    aug = _aug(noise=bank, rirs=rirs, p_reverb=1.0, normalize=True)
    snr, start, ridx = [5.0, 0.0, 9999.0, 15.0], [0, 11, 0, bank.size - lens[3]], [0, 1, 1, -1]
    x = torch.from_numpy(sig).to(DEV)

    def embed(wave):
        feats, nf = fe(wave, lens)
        return net.extract_embedding(feats, lengths=nf)[0].cpu().numpy()

    got = embed(aug(x, lens, params=_params(snr=snr, start=start, ridx=ridx)))
    host = np.stack([ref_row(sig[b], n, rir=None if ridx[b] < 0 else (rirs[ridx[b]], RIR_PEAKS[pick[ridx[b]]][1]), bank=bank, start=start[b],
                             snr=snr[b], normalize=True) for b, n in enumerate(lens)]).astype(np.float32)
    want = embed(torch.from_numpy(host).to(DEV))
    plain = embed(x)
    e = rel_err(got, want)
    print(f"chain: rel_err {e:.3e}; augmented vs plain {rel_err(got, plain):.3e}")
    assert e < 1e-4
    assert rel_err(got, plain) > 1e-2                                                      # the stage is not a no-op


# --------------------------------------------------------------------------------------------------------------- 8. the trainer
def test_train_audio_from_waves_with_the_fft_route(tmp_path, monkeypatch, recwarn):
    import train_audio
    monkeypatch.chdir(tmp_path)
    augment = {"snr_levels": [0, 10, 9999], "p_reverb": 0.5, "keep_power": True, "normalize": False, "reverb": "fft"}
    torch.manual_seed(0)
    tr = train_audio.Trainer("conf/audio_config.yaml", overrides=dict(SMALL, **{"data.train_from_waves": True, "data.augment": augment}))
    try:
        assert tr._augment.reverb == "fft" and tr._augment.truncated == []
        assert tr._augment.rir.shape[1] > _lib.DLIP_FIR_MAX_TAPS                           # the long synthetic response, whole
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        st = dict(tr.last_epoch_stats)
    finally:
        tr.close()
    assert np.isfinite(loss) and np.isfinite(st["loss"])
    assert st["from_waves"] is True and st["augment"]["reverb"] == "fft" and st["augment"]["max_taps"] == _lib.DLIP_OLS_MAX_TAPS
    assert st["steps"] == 2 and st["bs"] == 8
    assert not [w for w in recwarn.list if "truncated" in str(w.message)]
