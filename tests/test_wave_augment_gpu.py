"""Waveform augmentation on the device (-m gpu): reverberation, additive noise at an SNR and utterance normalisation
(deeplip_amd/augment.py) against an fp64 restatement of the definition, at the FIR kernel's tile and tap-chunk
edges; the exact cases; each row as if alone; inside a recorded plan; in front of the front-end and an encoder; in train_audio's
``data.train_from_waves`` mode; the reference's two class names as drop-ins.

Geometry, with T = DLIP_FIR_TILE and K = DLIP_FIR_TAP_CHUNK: one batch padded to S = 2T + 3 samples whose rows hold
n = 2T + 3, 2T, T + 1, T, T - 1 and 1 samples; room responses of 1, 2, K, K + 1 and 2K + 5 taps with the direct path at tap 0, at the
last tap or mid-way.  Bars: the project's output bar rel_err < 2e-5 per row for the stages, the front-end's 1e-4 behind it."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from deeplip_amd import _lib, weightgen as wg
from test_models_gpu import DEV, load, tdnn_opts

pytestmark = pytest.mark.gpu

T, K = _lib.DLIP_FIR_TILE, _lib.DLIP_FIR_TAP_CHUNK
S = 2 * T + 3
LENS = (2 * T + 3, 2 * T, T + 1, T, T - 1, 1)
B = len(LENS)
RIR_PEAKS = ((1, 0), (2, 1), (K, K // 2), (K + 1, 0), (2 * K + 5, 2 * K + 4))           # (taps, direct-path tap)
BANK = 3 * T
BAR = 2e-5                                                                                # README, "project bars"


# ------------------------------------------------------------------------- the definition (ISSUE / DESIGN.md 4d), restated in fp64
def ref_reverb(x, h, d, keep_power):
    x, h = x.astype(np.float64), h.astype(np.float64)
    y = np.convolve(x, h)[d:d + x.size]                          # y[t] = sum_k h[k] x[t + d - k], x zero outside [0, n)
    if keep_power:
        px, py = np.mean(x ** 2), np.mean(y ** 2)
        y = y * (np.sqrt(px / py) if py > 0 else 1.0)
    return y


def ref_noise(y, bank, start, snr):
    y = y.astype(np.float64)
    c = bank[start:start + y.size].astype(np.float64)
    pc = np.mean(c ** 2)
    if snr >= 9999 or pc == 0:
        return y
    return y + c * np.sqrt((np.mean(y ** 2) / pc) / 10.0 ** (snr / 10.0))


def ref_normalize(z):
    z = z.astype(np.float64)
    sd = z.std()
    return (z - z.mean()) / sd if sd > 0 else np.zeros_like(z)


def ref_row(x, n, rir=None, bank=None, start=0, snr=9999, keep_power=True, normalize=False, stage32=True):
    """Row x[:n] through the configured stages -> [len(x)] with the zero tail.  Between two stages the device holds fp32."""
    f32 = (lambda v: v.astype(np.float32)) if stage32 else (lambda v: v)
    y = x[:n].astype(np.float64)
    if rir is not None:
        y = f32(ref_reverb(y, rir[0], rir[1], keep_power))
    if bank is not None:
        y = f32(ref_noise(y, bank, start, snr))
    if normalize:
        y = ref_normalize(y)
    out = np.zeros(x.size)
    out[:n] = y
    return out


# ------------------------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _signals():
    t = np.arange(S) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (210 + 140 * b) * t) + 0.05 * wg.gen(f"wa.sig{b}", (S,)) for b in range(B)]).astype(np.float32)
    sig.setflags(write=False)
    return sig


@functools.lru_cache(maxsize=None)
def _rirs():
    out = []
    for i, (n, p) in enumerate(RIR_PEAKS):
        h = 0.1 * wg.gen(f"wa.rir{i}", (n,))
        h[p] = 1.0 if i % 2 == 0 else -1.0
        h.setflags(write=False)
        out.append(h.astype(np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _bank():
    b = (0.2 * wg.gen("wa.bank", (BANK,))).astype(np.float32)
    b.setflags(write=False)
    return b


def _batch(fill=0.0, lens=LENS):
    x = np.full((len(lens), S), fill, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = _signals()[b, :n]
    return torch.from_numpy(x).to(DEV)


def _lens_dev(vals=LENS):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def _aug(**kw):
    from deeplip_amd.augment import WaveAugment
    return WaveAugment(**kw)


def _params(snr=None, start=None, ridx=None):
    p = {}
    if snr is not None:
        p["snr_db"] = np.asarray(snr, dtype=np.float32)
        p["noise_start"] = np.asarray(start if start is not None else [0] * len(snr), dtype=np.int64)
    if ridx is not None:
        p["rir_idx"] = np.asarray(ridx, dtype=np.int32)
    return p


SNRS = (-5.0, 0.0, 20.0, 9999.0, -5.0, 20.0)
STARTS = (BANK - LENS[0], 17, BANK - LENS[2], 5, 0, BANK - 1)        # row 0 and row 2 end exactly on the bank's last sample


# ----------------------------------------------------------------------------------------------------------- 1. FIR against fp64
@pytest.mark.parametrize("keep_power", [False, True])
def test_fir_against_fp64(keep_power):
    aug = _aug(rirs=_rirs(), p_reverb=1.0, keep_power=keep_power)
    assert aug.rir_len.tolist() == [n for n, _ in RIR_PEAKS] and aug.rir_peak.tolist() == [p for _, p in RIR_PEAKS]
    assert min(LENS) < min(n for n, _ in RIR_PEAKS if n > 1)                              # responses longer than the shortest row
    x = _batch()
    sig = _signals()
    worst = worst32 = 0.0
    for shift in range(len(RIR_PEAKS)):                                                    # every row meets every response
        ridx = [(b + shift) % len(RIR_PEAKS) for b in range(B)]
        y = aug(x, list(LENS), params=_params(ridx=ridx)).cpu().numpy()
        for b, n in enumerate(LENS):
            h, d = _rirs()[ridx[b]], RIR_PEAKS[ridx[b]][1]
            want = ref_row(sig[b], n, rir=(h, d), keep_power=keep_power)
            e = rel_err(y[b], want)
            # numpy's own float32 evaluation of the same sums: the bar measures the kernel, not the conditioning of the data
            y32 = np.convolve(sig[b, :n], h)[d:d + n]
            assert y32.dtype == np.float32
            e32 = rel_err(y32, ref_reverb(sig[b, :n], h, d, False))
            worst, worst32 = max(worst, e), max(worst32, e32)
            print(f"keep_power {keep_power} row {b} (n {n}) response {ridx[b]} ({h.size} taps, d {d}): rel_err {e:.3e}, numpy f32 {e32:.3e}")
            assert e32 < BAR / 4, (b, ridx[b])
            assert e < BAR, (b, ridx[b])
            assert not y[b, n:].any()
    print(f"worst rel_err {worst:.3e} (numpy float32: {worst32:.3e})")


# ------------------------------------------------------------------------------------------------------------- 2. exact cases
def test_exact_cases():
    x = _batch()
    clean = x.clone()
    for b, n in enumerate(LENS):
        clean[b, n:] = 0
    lens = list(LENS)
    # h = [1]; h = [0, 0, 1] read at its own tap d = 2: the input.  keep_power: the gain is sqrt(Px / Py) = 1 exactly.
    for keep_power in (False, True):
        aug = _aug(rirs=[np.array([1.0]), np.array([0.0, 0.0, 1.0])], p_reverb=1.0, keep_power=keep_power)
        assert aug.rir_peak.tolist() == [0, 2]
        for r in (0, 1):
            assert torch.equal(aug(x, lens, params=_params(ridx=[r] * B)), clean), (keep_power, r)
    # the same response with the direct path declared at tap 0: the input delayed by two samples, zeros shifted in
    aug = _aug(rirs=[np.array([0.0, 0.0, 1.0])], rir_peaks=[0], p_reverb=1.0, keep_power=False)
    y = aug(x, lens, params=_params(ridx=[0] * B))
    want = torch.zeros_like(clean)
    for b, n in enumerate(LENS):
        want[b, 2:n] = clean[b, :max(n - 2, 0)]
    assert torch.equal(y, want)
    # rows with rir_idx < 0 and rows at the sentinel are untouched, whatever the other rows do
    bank = np.concatenate([np.zeros(S, dtype=np.float32), _bank()])
    aug = _aug(noise=bank, rirs=_rirs(), p_reverb=0.5)
    ridx = [-1, 4, -1, 2, -1, -7]
    snr = [9999.0, 9999.0, 5.0, 9999.0, 9999.0, 10 ** 6]
    y = aug(x, lens, params=_params(snr=snr, start=[S] * B, ridx=ridx))
    for b in (0, 4, 5):
        assert torch.equal(y[b], clean[b]), b
    for b in (1, 2, 3):
        assert not torch.equal(y[b], clean[b]), b
    # a noise slice of zero power passes through (the reference divides by zero there)
    y = aug(x, lens, params=_params(snr=[0.0] * B, start=[0, 0, 0, S + 1, 0, S - 1], ridx=[-1] * B))
    for b in (0, 1, 2, 4, 5):
        assert torch.equal(y[b], clean[b]), b
    assert not torch.equal(y[3], clean[3])


def test_padding_is_never_read_and_the_tail_is_zero(monkeypatch):
    """1e30 and NaN behind the rows, NaN in every buffer the wrapper takes: the zero-padded run's output bit for bit, zeros at
    t >= n.  Device lengths outside [1, S] are clamped."""
    from deeplip_amd import ops
    real_empty = ops._empty

    def nan_empty(shape, device, dtype=torch.float32):
        return real_empty(shape, device, dtype).fill_(float("nan"))
    aug = _aug(noise=_bank(), rirs=_rirs(), p_reverb=1.0, normalize=True)
    p = _params(snr=SNRS, start=STARTS, ridx=[4, 3, 2, 1, 0, 2])
    want = aug(_batch(0.0), _lens_dev(), params=p)
    monkeypatch.setattr(ops, "_empty", nan_empty)
    outs = [aug(_batch(fill), _lens_dev(), params=p) for fill in (1e30, float("nan"))]
    monkeypatch.setattr(ops, "_empty", real_empty)
    for y in outs:
        assert torch.isfinite(y).all() and torch.equal(y, want)
        for b, n in enumerate(LENS):
            assert not y[b, n:].any() and (n == 1 or y[b, :n].any())
    clamped = [S, LENS[1], 1, LENS[3], 1, S]
    xb = _batch(lens=clamped)
    got = aug(xb, _lens_dev([S + 5, LENS[1], 0, LENS[3], -3, 10 ** 6]), params=p)
    assert torch.equal(got, aug(xb, clamped, params=p))


# --------------------------------------------------------------------------------------------------------- 3. noise against fp64
def test_noise_against_fp64():
    aug = _aug(noise=_bank())
    x = _batch()
    z = aug(x, list(LENS), params=_params(snr=SNRS, start=STARTS)).cpu().numpy()
    sig, bank = _signals(), _bank()
    assert STARTS[0] == len(bank) - LENS[0]
    for b, n in enumerate(LENS):
        want = ref_row(sig[b], n, bank=bank, start=STARTS[b], snr=SNRS[b])
        e = rel_err(z[b], want)
        print(f"row {b} (n {n}, {SNRS[b]} dB): rel_err {e:.3e}")
        assert e < BAR, b
        assert not z[b, n:].any()
        if SNRS[b] >= 9999:
            assert np.array_equal(z[b, :n], sig[b, :n])
            continue
        y = sig[b, :n].astype(np.float64)
        added = z[b, :n].astype(np.float64) - y
        got_db = 10.0 * np.log10(np.sum(y ** 2) / np.sum(added ** 2))
        print(f"    achieved {got_db:.6f} dB")
        assert abs(got_db - SNRS[b]) < 1e-3, (b, got_db)


# --------------------------------------------------------------------------------------------------------------- 4. normalisation
def test_normalisation():
    aug = _aug(normalize=True)
    x = _batch()
    x[3, :] = 0.37                                                                         # a constant row
    out = aug(x, list(LENS), params={}).cpu().numpy()
    xin = x.cpu().numpy()
    for b, n in enumerate(LENS):
        v = out[b, :n].astype(np.float64)
        assert not out[b, n:].any()
        if b == 3 or n == 1:
            assert not v.any(), b                                                          # std 0: zeros exactly
            continue
        print(f"row {b}: mean {v.mean():.3e}, var - 1 {v.var() - 1:.3e}")
        assert abs(v.mean()) < 1e-5 and abs(v.var() - 1.0) < 1e-5, b
        assert rel_err(v, ref_normalize(xin[b, :n])) < BAR, b


# ----------------------------------------------------------------------------------------------------- 5. each row as if alone
def test_each_row_equals_the_row_alone():
    aug = _aug(noise=_bank(), rirs=_rirs(), p_reverb=1.0, normalize=True)
    ridx = [4, 3, 2, 1, 0, 2]
    x = _batch(1e30)
    y = aug(x, _lens_dev(), params=_params(snr=SNRS, start=STARTS, ridx=ridx))
    sig = _signals()
    for b, n in enumerate(LENS):
        alone = aug(x[b:b + 1, :n].contiguous(), params=_params(snr=SNRS[b:b + 1], start=STARTS[b:b + 1], ridx=ridx[b:b + 1]))
        assert alone.shape == (1, n)
        assert torch.equal(y[b:b + 1, :n], alone), b
        want = ref_row(sig[b], n, rir=(_rirs()[ridx[b]], RIR_PEAKS[ridx[b]][1]), bank=_bank(), start=STARTS[b], snr=SNRS[b], normalize=True)
        if n > 1:
            assert rel_err(y[b].cpu().numpy(), want) < BAR, b


# ------------------------------------------------------------------------------------------------------------------ 6. recorded
def test_a_recorded_plan_follows_new_params_and_lengths():
    from deeplip_amd.plan import StepPlan
    aug = _aug(noise=_bank(), rirs=_rirs(), p_reverb=1.0, normalize=True)

    def step(wave, lens, snr, start, ridx):
        return aug(wave, lens, params={"snr_db": snr, "noise_start": start, "rir_idx": ridx})

    def inputs(fill, lens, snr, start, ridx):
        p = _params(snr=snr, start=start, ridx=ridx)
        return (_batch(fill), _lens_dev(lens)) + tuple(torch.from_numpy(p[k]).to(DEV) for k in ("snr_db", "noise_start", "rir_idx"))

    ins0 = inputs(0.0, LENS, SNRS, STARTS, [0, 1, 2, 3, 4, 0])
    plan = StepPlan(step, *ins0)
    first = plan.run().clone()
    torch.cuda.synchronize()
    assert torch.equal(first, step(*ins0))
    lens1 = (T, 1, 2 * T + 3, 77, 2 * T - 1, T + 9)
    ins1 = inputs(7.0, lens1, (9999.0, 3.0, 10.0, 0.0, 9999.0, -5.0), (0, 9, 1, 2 * T, 0, 100), [4, -1, 3, 2, -1, 1])
    got = plan(*ins1).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, step(*ins1)) and not torch.equal(got, first)
    print(f"launches in the plan: {plan.launches}")
    assert plan.launches == 6                                                            # reverb 2 (keep_power), noise 2, normalise 2
    plan.close()


# ----------------------------------------------------------------------------------------------------------------- 7. the chain
def test_the_chain_into_frontend_and_encoder():
    from deeplip_amd.frontend import AudioFrontend
    from models.audio_models.tdnn import SpeakerEmbNet
    net, _ = load(SpeakerEmbNet(tdnn_opts()), "wa.chain.")
    fe = AudioFrontend("mfcc")
    lens = [400 + 39 * 160, 6000, 5000, 4100]                                             # 40, 36, 30, 25 frames
    Sp = lens[0]
    t = np.arange(Sp) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (180 + 90 * b) * t) + 0.05 * wg.gen(f"wa.chain.{b}", (Sp,)) for b in range(4)]).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0
    rirs, bank = _rirs()[2:4], (0.2 * wg.gen("wa.chain.bank", (8000,))).astype(np.float32)
    aug = _aug(noise=bank, rirs=rirs, p_reverb=1.0)
    snr, start, ridx = [5.0, 0.0, 9999.0, 15.0], [0, 11, 0, bank.size - lens[3]], [0, 1, 1, -1]
    x = torch.from_numpy(sig).to(DEV)

    def embed(wave):
        feats, nf = fe(wave, lens)
        return net.extract_embedding(feats, lengths=nf)[0].cpu().numpy()

    got = embed(aug(x, lens, params=_params(snr=snr, start=start, ridx=ridx)))
    host = np.stack([ref_row(sig[b], n, rir=None if ridx[b] < 0 else (rirs[ridx[b]], RIR_PEAKS[2 + ridx[b]][1]), bank=bank, start=start[b],
                             snr=snr[b]) for b, n in enumerate(lens)]).astype(np.float32)
    want = embed(torch.from_numpy(host).to(DEV))
    plain = embed(x)
    e = rel_err(got, want)
    print(f"chain: rel_err {e:.3e}; augmented vs plain {rel_err(got, plain):.3e}")
    assert e < 1e-4
    assert rel_err(got, plain) > 1e-2                                                      # the stage is not a no-op


# --------------------------------------------------------------------------------------------------------------- 8. the trainer
SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.audio_frames": 60, "data.test_speakers": 2, "data.test_utt_per_spk": 2,
         "model.arch": "tdnn", "model.tdnn": tdnn_opts()["tdnn"], "train.bs": 8, "train.steps_per_epoch": 2, "train.crop_frames": [40, 48]}
AUGMENT = {"snr_levels": [0, 10, 9999], "p_reverb": 0.5, "keep_power": True, "normalize": False, "max_taps": 8192}


def _epoch(overrides, config="conf/audio_config.yaml"):
    import train_audio
    torch.manual_seed(0)                    # the criterion's weights come from torch's generator (nn.init in LMCL)
    tr = train_audio.Trainer(config, overrides=dict(SMALL, **overrides))
    try:
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        return loss, dict(tr.last_epoch_stats)
    finally:
        tr.close()


def test_train_audio_from_augmented_waves(tmp_path, monkeypatch):
    import yaml
    monkeypatch.chdir(tmp_path)
    # the parent's path, twice: a config without the new keys at all, and the shipped one with train_from_waves: False
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        conf = yaml.safe_load(f)
    assert conf["data"].pop("train_from_waves") is False and "augment" not in conf["data"]
    bare = tmp_path / "audio_config_bare.yaml"
    bare.write_text(yaml.safe_dump(conf))
    one = {"train.steps_per_epoch": 1}
    l_bare, s_bare = _epoch(one, config=str(bare))
    l_off, s_off = _epoch(dict(one, **{"data.train_from_waves": False}))
    assert l_bare == l_off and np.isfinite(l_bare)
    assert "from_waves" not in s_off and "augment" not in s_off and sorted(s_off) == sorted(s_bare)
    loss, st = _epoch({"data.train_from_waves": True, "data.augment": dict(AUGMENT)})
    assert np.isfinite(loss) and np.isfinite(st["loss"])
    assert st["from_waves"] is True and st["augment"]["p_reverb"] == 0.5 and st["augment"]["snr_levels"] == (0.0, 10.0, 9999.0)
    assert st["steps"] == 2 and st["bs"] == 8
    # the step behind the new stages is the recorded one, as on the feature path: first meeting of a crop length eager, then its graph
    # (never "eager: <why the recorded step was dropped>"); which of the two the epoch ends on depends on the crop lengths drawn
    assert s_off["step_mode"] == "eager (warm-up)" and st["step_mode"] in ("eager (warm-up)", "graph")
    assert st["crop_ladder"] == s_off["crop_ladder"] and 40 <= min(st["crop_ladder"]) <= max(st["crop_ladder"]) <= 48
    loss_w, st_w = _epoch({"data.train_from_waves": True})                                # waveforms without augmentation
    assert np.isfinite(loss_w) and st_w["from_waves"] is True and st_w["augment"] is None and loss_w != loss


# --------------------------------------------------------------------------------------------------------------- 9. the drop-ins
def _reference_add_noise(noise, levels, signal):
    """models/video_models/preprocess.py:165-178 on float64 copies."""
    snr_target = random.choice(levels)
    if snr_target == 9999:
        return signal
    start_idx = random.randint(0, len(noise) - len(signal))
    noise_clip = noise[start_idx:start_idx + len(signal)].astype(np.float64)
    sig = signal.astype(np.float64)
    factor = (np.mean(sig ** 2) / np.mean(noise_clip ** 2)) / (10 ** (snr_target / 10.0))
    return sig + noise_clip * np.sqrt(factor)


def test_drop_in_classes():
    from models.video_models.preprocess import AddNoise, NormalizeUtterance
    levels = [-5, 0, 5, 10, 15, 20, 9999]
    noise, sig = _bank(), _signals()
    t = AddNoise(noise, levels)
    signals = [sig[0, :3000], sig[1], sig[2, :T + 1], sig[3, :500]]
    random.seed(3)
    want = [_reference_add_noise(noise, levels, s) for s in signals]
    state = random.getstate()
    random.seed(3)
    got = [t(torch.from_numpy(s.copy()).to(DEV)) for s in signals]
    assert random.getstate() == state
    mixed = 0
    for g, w, s in zip(got, want, signals):
        assert g.shape == (s.size,) and g.is_cuda
        assert rel_err(g.cpu().numpy(), w) < BAR
        mixed += not np.array_equal(w, s)
    assert mixed >= 1                                                                      # (a level below 9999 came up)
    # a batch draws once per row, in row order
    random.seed(5)
    snr, start = t.draw(list(LENS))
    random.seed(5)
    zb = t(_batch(), lengths=list(LENS)).cpu().numpy()
    for b, n in enumerate(LENS):
        assert rel_err(zb[b], ref_row(sig[b], n, bank=noise, start=int(start[b]), snr=float(snr[b]))) < BAR, b
    norm = NormalizeUtterance()
    for s in signals:
        g = norm(torch.from_numpy(s.copy()).to(DEV))
        assert g.shape == (s.size,)
        assert rel_err(g.cpu().numpy(), (s.astype(np.float64) - np.mean(s.astype(np.float64))) / np.std(s.astype(np.float64))) < BAR
