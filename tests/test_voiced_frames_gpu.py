"""Sliding-window CMN and energy-VAD frame selection on the device (-m gpu): against the fp64 restatement of
tests/voiced_frames_ref.py, row by row; the VAD decision and the kept-frame counts exactly; ragged invariants (hostile padding, the
row run alone, full lengths); inside a recorded plan; through train_fusion's and train_audio's extraction.

Bars.  CMN: the project's output bar, max|got - ref| <= 2e-5 x the row's largest magnitude (about one fp32 rounding, 6e-8, is
expected: the sums are fp64 on both sides and the result is rounded once).  VAD: exact -- the inputs keep every frame's energy at
least 1e-3 away from the threshold (asserted from the restatement first), so a last-bit difference of the fp64 mean cannot flip a
decision.  Everything the device is compared with itself on (ragged rows, plans, selection vs no selection) is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import voiced_frames_ref as R
from conftest import rel_err
from deeplip_amd import _lib, weightgen as wg
from test_models_gpu import DEV

pytestmark = pytest.mark.gpu

TILE = _lib.DLIP_CMN_TILE
C_CMN = 3
BAR = 2e-5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lens(l):
    return torch.tensor(list(l), dtype=torch.int32, device=DEV)


def _stage(**kw):
    from deeplip_amd.voiced_frames import VoicedFrames
    return VoicedFrames(**kw)


# ------------------------------------------------------------------------------------------ 1. CMN against the restatement
def _cmn_lengths(window):
    return sorted({n for n in (1, 2, window - 1, window, window + 1, TILE - 1, TILE + 1, 2 * TILE + 3) if n >= 1})


@functools.lru_cache(maxsize=None)
def _row(n):
    """One utterance [C_CMN, n]: an offset per channel (a mean worth removing) + a slow drift + noise."""
    t = np.arange(n, dtype=np.float64)
    x = np.array([3.0, -40.0, 0.25])[:, None] + np.array([1.0, 5.0, 0.1])[:, None] * (np.sin(t / 97.0)[None] + wg.gen(f"vf.row{n}", (C_CMN, n)))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _cmn_ref(n, window, center, norm_vars):
    out = R.cmn(_row(n), window, center, 100, norm_vars)
    out.setflags(write=False)
    return out


def _cmn_batch(window, NF):
    ns = _cmn_lengths(window)
    x = np.full((len(ns), C_CMN, NF), np.nan, dtype=np.float32)       # hostile padding: never loaded
    for b, n in enumerate(ns):
        x[b, :, :n] = _row(n)
    return ns, _dev(x)


def _check_cmn(window, center, norm_vars, NF):
    ns, x = _cmn_batch(window, NF)
    y, out_len = _stage(cmn_window=window, center=center, norm_vars=norm_vars, vad=None)(x, ns)
    assert out_len.tolist() == ns
    y = y.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(ns):
        ref = _cmn_ref(n, window, center, norm_vars)
        assert not y[b, :, n:].any(), (b, n)                          # the tail: exact zeros
        for c in range(C_CMN):
            top = float(np.abs(ref[c]).max())
            err = float(np.abs(y[b, c, :n].astype(np.float64) - ref[c]).max())
            assert err <= BAR * top, (n, c, err, top)
            worst = max(worst, err / top) if top > 0 else worst
        if center and not norm_vars and n <= window:                  # the window is the whole utterance: plain mean removal
            x64 = _row(n).astype(np.float64)
            plain = (x64 - (np.cumsum(x64, axis=1)[:, -1] / n)[:, None]).astype(np.float32)
            assert np.array_equal(ref, plain)
            assert rel_err(y[b, :, :n], plain) <= BAR
    print(f"cmn window={window} center={center} norm_vars={norm_vars} NF={NF}: max relative error {worst:.3e}")


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("window", [1, 7, 300])
def test_cmn_equals_the_restatement(window, center, norm_vars):
    """Every length at which the window rule or the tiling takes another path, in one ragged batch with NaN padding; NF = 2 TILE + 3
    is no multiple of 4 (the scalar loads)."""
    _check_cmn(window, center, norm_vars, 2 * TILE + 3)


@pytest.mark.parametrize("norm_vars", [False, True])
def test_cmn_equals_the_restatement_on_the_vector_path(norm_vars):
    """NF a multiple of 4: float4 loads of whole quads inside the row's own frames, float4 stores."""
    _check_cmn(300, True, norm_vars, 2 * TILE + 4)


# ------------------------------------------------------------------------------------------ 2. the VAD decision, exactly
VAD_LENS = (1, 2, 5, 257, 700, 1023, 1024, 1025, 2100)                 # around a thread's four frames and the scan's 1024-frame chunks
VAD_NF = 2100


@functools.lru_cache(maxsize=None)
def _energy(n, kind="mixed"):
    """[n] float32 log-energies: speech frames in [8, 12], silence in [-2, 2] (runs of random length), far from any threshold the
    tests place between them."""
    r = np.random.Generator(np.random.PCG64([wg.DEFAULT_SEED & 0xFFFFFFFF, n, {"mixed": 0, "speech": 1}[kind]]))
    if kind == "speech":
        speech = np.ones(n, dtype=bool)
    else:
        speech = np.zeros(n, dtype=bool)
        t, on = 0, bool(r.integers(0, 2))
        while t < n:
            k = int(r.integers(1, 9))
            speech[t:t + k] = on
            t, on = t + k, not on
    e = np.where(speech, r.uniform(8.0, 12.0, n), r.uniform(-2.0, 2.0, n)).astype(np.float32)
    e.setflags(write=False)
    return e


def _vad_batch(kind="mixed", lens=VAD_LENS, NF=VAD_NF):
    """x [B, 3, NF]: row 0 the frame index (what is left of it tells which frames were kept), row 1 the energy, row 2 noise."""
    x = np.full((len(lens), 3, NF), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, 0, :n] = np.arange(n)
        x[b, 1, :n] = _energy(n, kind)
        x[b, 2, :n] = wg.gen(f"vf.vad{n}", (n,))
    return x


def _run_selection(x, lens, vad, min_keep=1, **call):
    st = _stage(cmn_window=None, vad=vad, energy_row=1, min_keep=min_keep)
    y, out_len = st(_dev(x), list(lens), **call)
    return y.cpu().numpy(), out_len.tolist(), st.last_fallback.tolist()


def _check_selection(x, lens, y, out_len, fallback, voiced, min_keep):
    for b, n in enumerate(lens):
        want, k, fb = R.select(x[b, :, :n], voiced[b], min_keep)
        assert (out_len[b], fallback[b]) == (k, fb), (b, n)
        kept = y[b, 0, :k].astype(np.int64)                                              # the device's mask, read off the index row
        assert np.array_equal(kept, np.flatnonzero(voiced[b]) if not fb else np.arange(n)), (b, n)
        assert np.array_equal(y[b, :, :n], want) and not y[b, :, n:].any(), (b, n)       # a gather of x, zeros behind


@pytest.mark.parametrize("context,proportion", [(0, 0.12), (2, 0.12), (2, 0.6), (5000, 0.12), (5000, 0.6)])
def test_vad_decision_and_lengths_equal_the_restatement(context, proportion):
    """context 0, 2 and >= n; proportion 0.12 (the recipe's) and 0.6 (Kaldi's default: with context 2 the product 5 * 0.6f rounds to
    exactly 3 in fp32, so three voiced frames of five decide 'voiced' -- the fp64 product would not)."""
    x = _vad_batch()
    opts = {"energy_threshold": 2.5, "energy_mean_scale": 0.5, "frames_context": context, "proportion_threshold": proportion}
    voiced = []
    for n in VAD_LENS:
        v, thr, margin = R.vad(_energy(n), 2.5, 0.5, context, proportion)
        assert margin >= 1e-3, (n, thr, margin)                        # nothing lies close enough to the threshold to be argued about
        voiced.append(v)
    # (a context >= n votes on the whole row: all of it voiced at 0.12, the long rows unvoiced -- the fallback -- at 0.6)
    assert context > 2 or any(v.any() and not v.all() for v in voiced)
    y, out_len, fallback = _run_selection(x, VAD_LENS, opts)
    _check_selection(x, VAD_LENS, y, out_len, fallback, voiced, 1)
    # the same energies as an explicit [B, NF] vector
    e = np.ascontiguousarray(x[:, 1, :])
    y2, out_len2, fallback2 = _run_selection(x, VAD_LENS, opts, log_energy=_dev(e))
    assert np.array_equal(y, y2, equal_nan=True) and out_len2 == out_len and fallback2 == fallback


def test_vad_all_voiced_none_voiced_and_the_min_keep_boundary():
    lens = (5, 257, 700)
    x = _vad_batch("speech", lens)
    base = {"energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}
    # all voiced: thr = 0 + 0.5 * mean ~ 5, every energy in [8, 12]
    voiced = [R.vad(_energy(n, "speech"), 0.0, 0.5, 2, 0.12) for n in lens]
    assert all(v.all() and m >= 1e-3 for v, _, m in voiced)
    y, out_len, fallback = _run_selection(x, lens, dict(base, energy_threshold=0.0))
    assert out_len == list(lens) and fallback == [0, 0, 0]
    _check_selection(x, lens, y, out_len, fallback, [v for v, _, _ in voiced], 1)
    # none voiced: Kaldi would drop the utterance; here the row keeps every frame and says so
    voiced = [R.vad(_energy(n, "speech"), 100.0, 0.5, 2, 0.12) for n in lens]
    assert all(not v.any() and m >= 1e-3 for v, _, m in voiced)
    y, out_len, fallback = _run_selection(x, lens, dict(base, energy_threshold=100.0))
    assert out_len == list(lens) and fallback == [1, 1, 1]
    _check_selection(x, lens, y, out_len, fallback, [v for v, _, _ in voiced], 1)
    # V = min_keep - 1 falls back, V = min_keep does not
    x = _vad_batch("mixed", (700,))
    v, _, margin = R.vad(_energy(700), 2.5, 0.5, 0, 0.12)
    V = int(v.sum())
    assert margin >= 1e-3 and 1 < V < 700
    opts = {"energy_threshold": 2.5, "energy_mean_scale": 0.5, "frames_context": 0, "proportion_threshold": 0.12}
    for keep, want in ((V, (V, 0)), (V + 1, (700, 1))):
        y, out_len, fallback = _run_selection(x, (700,), opts, min_keep=keep)
        assert (out_len[0], fallback[0]) == want
        _check_selection(x, (700,), y, out_len, fallback, [v], keep)


def test_an_external_mask_decides_instead():
    x = _vad_batch()
    r = np.random.Generator(np.random.PCG64(7))
    mask = r.choice(np.array([0, 0, 1, 7], dtype=np.uint8), size=(len(VAD_LENS), VAD_NF))      # any non-zero byte means voiced
    mask[0, 0] = 0                                                                          # a one-frame row without a voiced frame
    voiced = [mask[b, :n] != 0 for b, n in enumerate(VAD_LENS)]
    y, out_len, fallback = _run_selection(x, VAD_LENS, {}, voiced=_dev(mask))      # (the VAD options are not read)
    assert fallback[0] == 1
    _check_selection(x, VAD_LENS, y, out_len, fallback, voiced, 1)
    yb, out_len_b, _ = _run_selection(x, VAD_LENS, {}, voiced=_dev(mask != 0))             # ... or a bool tensor
    assert np.array_equal(y, yb, equal_nan=True) and out_len_b == out_len


# ------------------------------------------------------------------------------------------ 3. selection behind the CMN
@pytest.mark.parametrize("norm_vars", [False, True])
def test_selected_columns_are_the_cmn_output_at_the_voiced_frames(norm_vars):
    """CMN runs over all n frames BEFORE the selection: the kept columns hold the bits of the CMN-only output at the voiced positions."""
    lens = (2 * TILE + 3, TILE + 1, 301, 64)
    x = _vad_batch("mixed", lens, 2 * TILE + 4)
    xd = _dev(x)
    opts = {"energy_threshold": 2.5, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}
    both = _stage(cmn_window=300, norm_vars=norm_vars, vad=opts, energy_row=1)
    y, out_len = both(xd, list(lens))
    plain, plain_len = _stage(cmn_window=300, norm_vars=norm_vars, vad=None)(xd, list(lens))
    y, plain = y.cpu().numpy(), plain.cpu().numpy()
    assert plain_len.tolist() == list(lens) and both.last_fallback.tolist() == [0] * len(lens)
    for b, n in enumerate(lens):
        v = R.vad(_energy(n), 2.5, 0.5, 2, 0.12)[0]
        k = int(v.sum())
        assert out_len[b].item() == k and 0 < k < n
        assert np.array_equal(y[b, :, :k], plain[b][:, :n][:, v]) and not y[b, :, k:].any(), (b, n)


# ------------------------------------------------------------------------------------------ 4. ragged invariants
RAGGED = {1: ((2049,), 2052), 5: ((2500, 2049, 301, 37, 1), 2500)}


@pytest.mark.parametrize("C", [1, 24])
@pytest.mark.parametrize("B", [1, 5])
def test_a_padded_row_equals_the_row_alone(B, C):
    """Row b of a padded batch (NaN padding, arbitrary neighbours; NF a multiple of 4: the float4 path) is bit-identical to the row
    run alone at its own length (mostly no multiple of 4: the scalar path)."""
    lens, NF = RAGGED[B]
    x = np.full((B, C, NF), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :, :n] = 3.0 * wg.gen(f"vf.rag{B}.{C}.{b}", (C, n)) + 1.0
    xd = _dev(x)
    opts = {"energy_threshold": 0.0, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.6}
    for kw in (dict(cmn_window=300, vad=opts), dict(cmn_window=7, center=False, min_window=3, norm_vars=True, vad=opts, min_keep=24),
               dict(cmn_window=300, vad=None), dict(cmn_window=None, vad=opts)):
        st = _stage(**kw)
        y, out_len = st(xd, list(lens))
        fb = None if st.last_fallback is None else st.last_fallback.tolist()
        assert torch.equal(y, st(xd, _lens(lens))[0])                  # host lengths and a device vector: the same call
        y = y.cpu().numpy()
        for b, n in enumerate(lens):
            ya, la = st(xd[b:b + 1, :, :n].contiguous())
            k = la.item()
            assert out_len[b].item() == k and (fb is None or st.last_fallback.item() == fb[b]), (kw, b)
            assert np.array_equal(y[b, :, :n], ya.cpu().numpy()[0]) and not y[b, :, n:].any(), (kw, b)
            assert not y[b, :, k:].any()


def test_full_lengths_equal_no_lengths():
    x = _dev(2.0 * wg.gen("vf.full", (3, 24, TILE + 4)) + 0.5)
    opts = {"energy_threshold": 0.0, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}
    for kw in (dict(cmn_window=300, vad=opts), dict(cmn_window=300, vad=None), dict(cmn_window=None, vad=opts)):
        st = _stage(**kw)
        y0, l0 = st(x)
        y1, l1 = st(x, [TILE + 4] * 3)
        assert torch.equal(y0, y1) and torch.equal(l0, l1) and torch.isfinite(y0).all(), kw


def test_a_device_length_vector_is_clamped_on_the_device():
    """Host lengths are validated; a device vector is never read on the host, so the kernels clamp it to [1, NF] themselves."""
    NF = 300
    x = _dev(wg.gen("vf.clamp", (4, 3, NF)))
    opts = {"energy_threshold": 0.0, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.6}
    for kw in (dict(cmn_window=300, vad=opts), dict(cmn_window=7, vad=None), dict(cmn_window=None, vad=opts)):
        st = _stage(**kw)
        y, l = st(x, _lens([0, -5, NF + 100, 17]))
        y2, l2 = st(x, [1, 1, NF, 17])
        assert torch.equal(y, y2) and torch.equal(l, l2), kw
    with pytest.raises(ValueError):
        _stage()(x, [0, 1, NF, 17])
    with pytest.raises(TypeError):
        _stage()(x, torch.tensor([1, 1, NF, 17], dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------ 5. a recorded plan
@pytest.mark.parametrize("vad", [True, False])
def test_the_stage_records_into_a_step_plan(vad):
    """Recorded once; the replay on a second batch and a second length vector equals the eager call bit for bit -- a data-dependent
    length is only another device vector."""
    from deeplip_amd.plan import StepPlan
    opts = {"energy_threshold": 0.0, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12} if vad else None
    st = _stage(cmn_window=300, vad=opts, min_keep=3)
    B, C, NF = 4, 24, TILE + 40

    def step(x, lens):
        return st(x, lens)

    ins0 = (_dev(wg.gen("vf.plan0", (B, C, NF))), _lens([NF, 700, 301, 2]))
    plan = StepPlan(step, *ins0)
    y0, l0 = (t.clone() for t in plan.run())
    torch.cuda.synchronize()
    e0 = step(*ins0)
    assert torch.equal(y0, e0[0]) and torch.equal(l0, e0[1])
    ins1 = (_dev(2.0 * wg.gen("vf.plan1", (B, C, NF)) - 1.0), _lens([5, NF, TILE + 1, 299]))
    y1, l1 = (t.clone() for t in plan(*ins1))
    torch.cuda.synchronize()
    e1 = step(*ins1)
    assert torch.equal(y1, e1[0]) and torch.equal(l1, e1[1]) and not torch.equal(l1, l0)
    if vad:
        assert (l1.cpu() < torch.tensor([5, NF, TILE + 1, 299])).any()
    plan.close()


# ------------------------------------------------------------------------------------------ 6. the entry points
SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
         "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
         "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False}
SILENT = 3000                                                          # samples of digital silence in front of every second utterance


def test_av_test_from_waveforms_with_voiced_frames(tmp_path, monkeypatch):
    """train_fusion's av_test, --from-waves with data.python_data_config.voiced_frames: every x-vector is front-end -> stage -> encoder
    of the utterance alone (the 1e-4 parity bar); the utterances with a silent head lose frames to the VAD.  The waveforms are floats
    around 1, so their log-energies sit near 6 where Kaldi's 16-bit samples sit near 18: the threshold is placed accordingly."""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    section = {"vad": {"energy_threshold": -5.0}}
    tr = train_fusion.Trainer("av_test", overrides=dict(SMALL, **{"data.python_data_config.test_from_waves": True,
                                                                  "data.python_data_config.voiced_frames": section}))
    try:
        ds = tr.lomgridtestset
        item = ds.wave_item

        def silenced(i, *a, **k):
            w = item(i, *a, **k).copy()
            if i % 2 == 0:
                w[:SILENT] = 0.0
            return w
        ds.wave_item = silenced
        tr.extract_test_xv_lomgrid()
        xa = tr.lomgrid_tables[1].emb
        assert torch.isfinite(tr.lomgrid_tables[0].emb).all()
        fe = tr._test_frontend("etdnn")
        assert fe.normalize is False                                   # the sliding mean replaces the utterance CMVN
        stage = tr._voiced_frames_stage(tr.model_audio.frames_consumed() + 2)
        assert stage.min_keep == tr.model_audio.frames_consumed() + 2 and stage.cmn_window == 300
        shorter = 0
        for i in range(len(ds)):
            feats = fe(torch.from_numpy(ds.wave_item(i)[None]).to(tr.device))
            y, ol = stage(feats)
            n, k = feats.shape[2], ol.item()
            assert stage.last_fallback.item() == 0 and (k < n if i % 2 == 0 else k <= n), (i, n, k)
            shorter += k < n
            want = tr.model_audio.extract_embedding(y, lengths=ol)[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-4, i
        assert shorter >= len(ds) // 2
    finally:
        tr.close()


def test_train_audio_extraction_with_voiced_frames(tmp_path, monkeypatch):
    """train_audio's ragged extraction (the `nn_input` pipe on feature-fed lists) with data.voiced_frames: every row is stage ->
    encoder of the utterance alone; a rectangular list is refused."""
    import train_audio
    monkeypatch.chdir(tmp_path)
    section = {"vad": {"energy_threshold": 0.0, "energy_mean_scale": 1.0, "frames_context": 0, "proportion_threshold": 0.6}}      # thr = the mean
    ov = {"data.test_speakers": 3, "data.test_utt_per_spk": 3, "data.trials": 60, "data.trial_targets": 12, "data.n_spk": 6,
          "data.utt_per_spk": 2, "data.test_audio_frames": [60, 140], "test.write_store": False, "data.voiced_frames": section}
    tr = train_audio.Trainer(overrides=ov)
    try:
        ds = tr.voxtestset
        assert ds.ragged
        table = tr._xvectors(ds, batch=4, normalize=False)
        stage = tr._voiced_frames_stage()
        assert stage.min_keep == tr._min_frames()
        ce = tr.train_opts["loss"] == "CrossEntropy"
        shorter = 0
        for i in range(len(ds)):
            x = torch.from_numpy(ds.audio_item(i)[None]).to(tr.device)
            y, ol = stage(x)
            shorter += ol.item() < x.shape[2]
            xv, x_a = tr.model.extract_embedding(y, lengths=ol)
            assert rel_err(table.emb[i:i + 1].cpu().numpy(), (x_a if ce else xv).cpu().numpy()) < 1e-4, i
        assert shorter >= 1
        ds.ragged = False
        with pytest.raises(ValueError, match="voiced_frames"):
            tr._xvectors(ds, batch=4)
    finally:
        tr.close()
