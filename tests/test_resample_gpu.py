"""Waveform resampling on the device (-m gpu; deeplip_amd/resample.py): the kernel against the fp64 restatement of
the definition (tests/resample_ref.py) on the fp32-rounded taps and inputs, output by output within the forward error bound of a K-term
fma chain; bit identity of a row whatever the batch, the bank, the output width and the neighbours are; a mixed bank; indices past
2^31; device lengths (clamped) and a recorded plan; train_audio's ``data.speed_perturb`` and train_fusion's ``source_rate``.

Geometry: B = 5 rows padded to S = 2500 samples holding 2500, 1 and 7 samples (one sample; shorter than the filter's half length) and
the two lengths either side of the kernel's first tile edge (the longest row whose outputs fill one tile of Resample.tile outputs, and
one sample more; 1024 and 2049 where the ratio puts that edge past S)."""
import functools
import os

import numpy as np
import pytest
import torch

import resample_ref as ref
from conftest import ROOT, rel_err
from deeplip_amd import weightgen as wg
from test_models_gpu import DEV, tdnn_opts

pytestmark = pytest.mark.gpu

B, S = 5, 2500
RATIOS = ((1, 3), (3, 1), (2, 3), (10, 9), (10, 11), (160, 441), (441, 160))
EPS = 2.0 ** -24


def _rs(up, down, **kw):
    from deeplip_amd.resample import Resample
    return Resample(down, up, **kw)                  # orig_rate -> new_rate: the ratio new / orig = up / down


def _lens(up, down):
    from deeplip_amd.resample import in_len
    T = _rs(up, down).tile
    hi = in_len(T + 1, up, down)                     # the shortest row that reaches into the second tile
    return [S, 1, 7] + ([hi - 1, hi] if 7 < hi - 1 and hi <= S else [1024, 2049])


@functools.lru_cache(maxsize=None)
def _signals():
    t = np.arange(S) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (210 + 140 * b) * t) + 0.05 * wg.gen(f"rs.sig{b}", (S,)) for b in range(B)]).astype(np.float32)
    sig.setflags(write=False)
    return sig


def _batch(lens, fill=0.0):
    x = np.full((len(lens), S), fill, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = _signals()[b, :n]
    return torch.from_numpy(x).to(DEV)


def _check_row(y, x, n, up, down, h, what, m=None):
    """y (the kernel's outputs ``m`` of the row x[:n]) against fp64 on the fp32-rounded taps, output by output:
    |y - y64| <= (K + 2) 2^-24 sum_i |x[i]| |h[...]|.  Returns the largest fraction of the bound used."""
    h32 = np.asarray(h, dtype=np.float32).astype(np.float64)
    K = -(-h32.size // up)
    want, scale = ref.resample(x[:n], up, down, h32, m=m, with_abs=True)
    err, bound = np.abs(np.asarray(y, dtype=np.float64) - want), (K + 2) * EPS * scale
    assert (err <= bound).all(), (what, int(np.argmax(err - bound)), float(err.max()))
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("up,down", RATIOS)
def test_parity_with_the_definition(up, down):
    from deeplip_amd.resample import out_len
    rs = _rs(up, down)
    lens = _lens(up, down)
    y, ol = rs(_batch(lens), lens)
    assert y.shape == (B, out_len(S, up, down)) and ol.dtype == torch.int32 and ol.is_cuda
    assert ol.tolist() == [out_len(n, up, down) for n in lens]
    y = y.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        no = out_len(n, up, down)
        assert not y[b, no:].any(), b                                                      # exact zeros past n_out
        worst = max(worst, _check_row(y[b, :no], _signals()[b], n, up, down, rs.h, (up, down, b)))
    print(f"{up}/{down} (tile {rs.tile}, lengths {lens}): largest fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441)])
def test_parity_across_tiles_when_decimating(up, down):
    """The decimating ratios put the first tile edge past S = 2500 inputs: one row of 7000 samples (three tiles of outputs), no lengths."""
    from deeplip_amd.resample import out_len
    rs = _rs(up, down)
    n = 7000
    x = (0.3 * np.sin(2 * np.pi * 0.013 * np.arange(n)) + 0.05 * wg.gen("rs.long", (n,))).astype(np.float32)
    y, ol = rs(torch.from_numpy(x[None]).to(DEV))
    assert ol.tolist() == [out_len(n, up, down)] and y.shape == (1, out_len(n, up, down)) and y.shape[1] > 2 * rs.tile
    frac = _check_row(y[0].cpu().numpy(), x, n, up, down, rs.h, (up, down))
    print(f"{up}/{down}, {n} samples: largest fraction of the bound {frac:.3f}")


# -------------------------------------------------------------------------------------------------------------- 2. bit identity
@pytest.mark.parametrize("up,down", [(1, 3), (10, 9), (160, 441), (441, 160)])
def test_each_row_equals_the_row_alone(up, down):
    from deeplip_amd.resample import out_len
    rs = _rs(up, down)
    lens = _lens(up, down)
    x = _batch(lens, fill=1e30)                                                            # the padding is never read
    y, ol = rs(x, torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert torch.isfinite(y).all() and torch.equal(y, rs(_batch(lens, fill=float("nan")), lens)[0])
    for b, n in enumerate(lens):
        alone, la = rs(x[b:b + 1, :n].contiguous())
        no = out_len(n, up, down)
        assert alone.shape == (1, no) and la.tolist() == [no] and int(ol[b]) == no
        assert torch.equal(y[b:b + 1, :no], alone), b


def test_bank_size_output_width_and_pass_through_leave_the_bits():
    from deeplip_amd.resample import SpeedPerturb, out_len
    lens = [S, 1, 7, 1024, 2049]
    x = _batch(lens)
    sp = SpeedPerturb((0.9, 1.0, 1.1))
    for k, (up, down) in ((0, (10, 9)), (2, (10, 11))):
        one, l1 = _rs(up, down)(x, lens)                                                   # a bank of Q = 1
        three, l3 = sp(x, lens, params={"speed_idx": np.full(B, k, dtype=np.int32)}, out_samples=one.shape[1])
        assert torch.equal(one, three) and torch.equal(l1, l3), (up, down)
        cut, lc = sp(x, lens, params={"speed_idx": np.full(B, k, dtype=np.int32)}, out_samples=300)
        assert cut.shape == (B, 300) and torch.equal(cut, one[:, :300].contiguous())
        assert lc.tolist() == [min(out_len(n, up, down), 300) for n in lens]
    clean = x.clone()
    for b, n in enumerate(lens):
        clean[b, n:] = 0
    for idx in (-1, 1, -7):                                                                # a negative index; the ratio 1/1 (h = [1.0])
        y, l = sp(_batch(lens, fill=7.0), lens, params={"speed_idx": np.full(B, idx, dtype=np.int32)}, out_samples=S)
        assert torch.equal(y, clean) and l.tolist() == lens, idx
    y, l = sp(x, lens, params={"speed_idx": np.full(B, -1, dtype=np.int32)}, out_samples=300)
    assert torch.equal(y, clean[:, :300].contiguous()) and l.tolist() == [min(n, 300) for n in lens]
    y, _ = sp(x, lens, params={"speed_idx": np.full(B, 1, dtype=np.int32)})              # the default width: the slowest speed's
    assert y.shape == (B, out_len(S, 10, 9)) and torch.equal(y[:, :S].contiguous(), clean) and not y[:, S:].any()


def test_a_mixed_bank_is_its_rows_alone():
    from deeplip_amd.resample import SpeedPerturb, out_len
    lens = [S, 1, 7, 1024, 2049]
    x = _batch(lens)
    sp = SpeedPerturb((0.9, 1.0, 1.1))
    idx = [0, 1, 2, 1, 0]
    W = sp.out_samples(S)
    y, l = sp(x, lens, params={"speed_idx": np.asarray(idx, dtype=np.int32)})
    assert y.shape == (B, W)
    single = [sp(x, lens, params={"speed_idx": np.full(B, k, dtype=np.int32)}) for k in range(3)]
    for b, k in enumerate(idx):
        assert torch.equal(y[b], single[k][0][b]) and int(l[b]) == int(single[k][1][b]) == out_len(lens[b], *sp.ratios[k]), b
    # an index past the bank is clamped to its last ratio, on the device
    yc, lc = sp(x, lens, params={"speed_idx": torch.full((B,), 9, dtype=torch.int32, device=DEV)})
    assert torch.equal(yc, single[2][0]) and torch.equal(lc, single[2][1])


# ----------------------------------------------------------------------------------------------------------- 3. 64-bit indexing
def test_indices_past_two_to_the_31():
    from deeplip_amd.resample import out_len
    up, down, n = 441, 160, 5_000_000
    assert n * up > 2 ** 31
    rs = _rs(up, down)
    g = np.random.Generator(np.random.PCG64(63))
    x = (0.3 * np.sin(2 * np.pi * 0.01 * np.arange(n)) + 0.05 * g.standard_normal(n)).astype(np.float32)
    y, ol = rs(torch.from_numpy(x[None]).to(DEV))
    no = out_len(n, up, down)
    assert y.shape == (1, no) and ol.tolist() == [no]
    m = np.concatenate([np.sort(g.choice(no - 2000, size=2000, replace=False)), np.arange(no - 2000, no)])
    got = y[0, torch.from_numpy(m).to(DEV)].cpu().numpy()
    frac = _check_row(got, x, n, up, down, rs.h, "5e6 samples at 441/160", m=m)
    print(f"441/160, {n} samples: largest fraction of the bound {frac:.3f}")


# ------------------------------------------------------------------------------------------- 4. device lengths and the step plan
def test_device_lengths_are_clamped_and_a_recorded_plan_follows_new_inputs():
    from deeplip_amd.plan import StepPlan
    from deeplip_amd.resample import SpeedPerturb
    rs = _rs(2, 3)
    sp = SpeedPerturb((0.9, 1.0, 1.1))
    clamped = [S, 1024, 1, 2049, 1]
    xb = _batch(clamped)
    wild = torch.tensor([S + 5, 1024, 0, 2049, -3], dtype=torch.int32, device=DEV)
    got, gl = rs(xb, wild)
    want, wl = rs(xb, clamped)
    assert torch.equal(got, want) and torch.equal(gl, wl)

    def step(wave, lens, idx):
        a, la = rs(wave, lens)
        b, lb = sp(wave, lens, params={"speed_idx": idx}, out_samples=S)
        return a, la, b, lb

    def inputs(lens, idx, fill):
        return (_batch(lens, fill), torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(idx, dtype=torch.int32, device=DEV))

    ins0 = inputs([S, 1, 7, 1024, 2049], [0, 1, 2, 1, 0], 0.0)
    plan = StepPlan(step, *ins0)
    first = [t.clone() for t in plan.run()]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, step(*ins0)))
    ins1 = inputs([77, S, 2049, 1, 1500], [2, -1, 0, 0, 1], 3.0)
    got = [t.clone() for t in plan(*ins1)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, step(*ins1))) and not torch.equal(got[0], first[0])
    print(f"launches in the plan: {plan.launches}")
    plan.close()


# --------------------------------------------------------------------------------------------------------------- 5. the trainers
SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.audio_frames": 60, "data.test_speakers": 2, "data.test_utt_per_spk": 2,
         "model.arch": "tdnn", "model.tdnn": tdnn_opts()["tdnn"], "train.bs": 8, "train.steps_per_epoch": 3, "train.crop_frames": [40, 40]}
AUGMENT = {"snr_levels": [0, 10, 9999], "p_reverb": 0.5, "keep_power": True, "normalize": False, "max_taps": 8192}
SPEEDS = {"speeds": [0.9, 1.0, 1.1]}


def _epoch(overrides):
    import train_audio
    torch.manual_seed(0)                    # the criterion's weights come from torch's generator (nn.init in LMCL)
    tr = train_audio.Trainer("conf/audio_config.yaml", overrides=dict(SMALL, **overrides))
    try:
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        return loss, dict(tr.last_epoch_stats)
    finally:
        tr.close()


def test_train_audio_with_speed_perturbation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain, st_plain = _epoch({"data.train_from_waves": True})
    none, st_none = _epoch({"data.train_from_waves": True, "data.speed_perturb": None})   # an absent and an empty section: one path
    assert plain == none and np.isfinite(plain) and "speed_perturb" not in st_plain and "speed_perturb" not in st_none
    for extra in ({}, {"data.augment": dict(AUGMENT)}):
        loss, st = _epoch(dict({"data.train_from_waves": True, "data.speed_perturb": dict(SPEEDS)}, **extra))
        assert np.isfinite(loss) and np.isfinite(st["loss"]) and loss != plain
        assert st["step_mode"] == "graph", st["step_mode"]                                 # the recorded step sees the same [B, F, T]
        assert st["speed_perturb"] == {"speeds": (0.9, 1.0, 1.1)} and st["from_waves"] is True
        assert (st["augment"] is None) == (not extra) and st["crop_ladder"] == st_plain["crop_ladder"] == [40]


FUSION_SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
                "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
                "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 16, "test.write_store": False}


def test_av_test_from_recordings_at_another_rate(tmp_path, monkeypatch):
    """train_fusion's av_test with ``source_rate: 48000`` in front of a 16 kHz front-end: each x-vector is the one of that utterance
    resampled alone and taken through the unresampled path (front-end, encoder), to the project's output bar."""
    import train_fusion
    from deeplip_amd.resample import Resample, ResampledGeometry
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("av_test", overrides=dict(FUSION_SMALL, **{"data.python_data_config.test_from_waves": True,
                                                                        "data.python_data_config.source_rate": 48000,
                                                                        "data.python_data_config.rate": 16000}))
    try:
        assert tr.source_rate == 48000
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        st = tr.extract_stats
        assert st["plans_recorded"] <= st["audio_shapes"] + st["video_shapes"]
        xa = tr.lomgrid_tables[1].emb
        assert torch.isfinite(tr.lomgrid_tables[0].emb).all()
        fe = tr._test_frontend("etdnn")
        rs = Resample(48000, 16000)
        g = ResampledGeometry(fe, rs)
        assert (g.frame_len, g.frame_step) == (1200, 480)
        worst = 0.0
        for i in range(len(ds)):
            w48 = torch.from_numpy(ds.wave_item(i, g.frame_len, g.frame_step)[None]).to(tr.device)
            w16, n16 = rs(w48)
            assert w16.shape[1] == rs.out_len(w48.shape[1]) == int(n16[0])
            want = tr.model_audio.extract_embedding(fe(w16))[0]
            e = rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy())
            worst = max(worst, e)
            assert e < 2e-5, (i, e)
        print(f"x-vectors of {len(ds)} resampled utterances: worst rel_err {worst:.3e}")
    finally:
        tr.close()
