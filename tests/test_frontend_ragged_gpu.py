"""The audio front-end on RAGGED waveform batches (-m gpu): a zero-padded batch + one sample count per row, each row computed as if
it had been run alone (AudioFrontend's ``lengths``) -- against the fp64 oracle of each utterance alone, with
hostile padding, against the row run alone on the GPU, inside a recorded plan, through RaggedExtractor.run(waves=True) and through
train_fusion's av_test.

Geometry: 16 kHz, 25 ms / 10 ms (400 / 160 samples), nfft 512; one batch padded to S = 2160 samples (12 frames):
    2160 -> 12 frames (full row) | 1999 -> 11 (last frame partly zero padding) | 401 -> 2 (just over one frame) |
    400 -> 1 (exactly one frame) | 123 -> 1 (shorter than one frame)
Bars: those tests/test_frontend.py holds the rectangular front-end to -- rel_err < 1e-4 per feature type (1e-4 with deltas), on the
bands it compares: after CMVN the bands whose variation over the utterance is above 1e-4 of the feature magnitude (the others are
normalised by a standard deviation the size of an fp32 ulp), and on the fp32 routes the un-normalised log elements above the -20
noise floor.  A one-frame utterance is all zeros after CMVN (std 0), exactly."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from deeplip_amd import weightgen as wg
from oracle import deeplip_oracle as O
from test_models_gpu import DEV, etdnn_opts, load

pytestmark = pytest.mark.gpu

S, LENS, NFS = 2160, (2160, 1999, 401, 400, 123), (12, 11, 2, 1, 1)
FEATS, ROUTES = ("mfcc", "fbank", "logfbank"), ("fft64", "gemm32", "direct64")
NUM_BIN = 26                      # (no empty mel filter at nfft 512: every band of every frame is compared)


@functools.lru_cache(maxsize=None)
def _signals():
    t = np.arange(S) / 16000.0
    sig = np.stack([0.3 * np.sin(2 * np.pi * (210 + 140 * b) * t) + 0.05 * wg.gen(f"fe.rag.n{b}", (S,)) for b in range(len(LENS))])
    sig = sig.astype(np.float32)
    sig.setflags(write=False)
    return sig


def _batch(fill=0.0):
    """[B, S]: row b = its utterance's first LENS[b] samples, ``fill`` behind them."""
    x = np.full((len(LENS), S), fill, dtype=np.float32)
    for b, n in enumerate(LENS):
        x[b, :n] = _signals()[b, :n]
    return torch.from_numpy(x).to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(b, feat, normalize, delta):
    """The oracle on utterance b ALONE: [F, NF_b]."""
    out = O.audio_features(_signals()[b, :LENS[b]].astype(np.float64), feat, nfilt=NUM_BIN, normalize=normalize, delta=delta)
    out.setflags(write=False)
    return out


def _frontend(feat, route, normalize=True, delta=False):
    from deeplip_amd.frontend import AudioFrontend
    fe = AudioFrontend(feat, num_bin=NUM_BIN, normalize=normalize, delta=delta, dft=route)
    assert fe.dft == route
    return fe


def _lens_dev(vals=LENS):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------ 1. against the oracle of each row alone
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("feat", FEATS)
def test_each_row_equals_the_oracle_of_that_utterance_alone(feat, route):
    x = _batch()
    for normalize in (False, True):
        for delta in (False, True):
            fe = _frontend(feat, route, normalize, delta)
            y, nf = fe(x, list(LENS))
            torch.cuda.synchronize()
            assert nf.dtype == torch.int32 and nf.is_cuda and nf.tolist() == list(NFS)
            assert y.shape == (len(LENS), fe.feat_dim, max(NFS))
            y = y.cpu().numpy()
            for b, n in enumerate(NFS):
                ref = _ref(b, feat, normalize, delta)
                assert ref.shape == (fe.feat_dim, n)                                  # frame_lengths == the oracle's frame counts
                got = y[b, :, :n]
                what = (feat, route, normalize, delta, b)
                raw = _ref(b, feat, False, False)
                if normalize and n == 1:
                    assert not ref.any() and not got.any(), what                      # std 0: 0 / 2e-12, deltas of zeros
                    continue
                keep = np.ones(ref.shape, bool)
                if normalize:
                    live = raw.std(axis=1) > 1e-4 * np.abs(raw).max()
                    assert live.sum() >= raw.shape[0] - 2, what
                    keep &= np.tile(live, ref.shape[0] // raw.shape[0])[:, None]
                elif route != "fft64" and feat == "logfbank":
                    keep &= np.tile(raw, (ref.shape[0] // raw.shape[0], 1)) >= -20.0   # (fp32 pre-emphasis: test_frontend.py's floor rule)
                e = float(np.abs((got - ref) * keep).max() / np.abs(ref * keep).max())
                print(f"{what}: rel_err {e:.3e} on {int(keep.sum())} of {keep.size} elements")
                assert e < 1e-4, what


# ------------------------------------------------------------------------------------------ 2. the padding is inert and defined
@pytest.mark.parametrize("route", ROUTES)
def test_padding_is_inert_and_every_padding_column_is_zero(route, monkeypatch):
    """NaN and 1e30 behind the utterances, NaN in every tensor the wrappers allocate (ops._empty: workspaces and outputs): the
    outputs are the zero-padded run's bit for bit, finite, and exactly 0.0 at t >= NF_b."""
    from deeplip_amd import ops
    real_empty = ops._empty

    def nan_empty(shape, device, dtype=torch.float32):
        t = real_empty(shape, device, dtype)
        return t.fill_(float("nan")) if dtype == torch.float32 else t.fill_(-7)
    for feat in FEATS:
        for normalize, delta in ((True, True), (False, False)):
            fe = _frontend(feat, route, normalize, delta)
            clean, nf0 = fe(_batch(0.0), _lens_dev())
            monkeypatch.setattr(ops, "_empty", nan_empty)
            outs = [fe(_batch(fill), _lens_dev()) for fill in (float("nan"), 1e30)]
            monkeypatch.setattr(ops, "_empty", real_empty)
            torch.cuda.synchronize()
            for y, nf in outs:
                assert torch.equal(nf, nf0) and nf.tolist() == list(NFS)
                assert torch.isfinite(y).all(), (feat, route, normalize)
                assert torch.equal(y, clean), (feat, route, normalize)
                for b, n in enumerate(NFS):
                    assert not y[b, :, n:].any(), (feat, route, normalize, b)
                    assert n == 1 and normalize or y[b, :, :n].any()


# ------------------------------------------------------------------------------------------ 3. a row alone vs the row in its batch
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("feat", FEATS)
def test_row_in_the_batch_equals_the_row_alone(feat, route):
    """Row b's valid columns == frontend(wave[b:b+1, :S_b]), BIT FOR BIT: framing, FFT, the matrix products and the log are per
    frame, and the CMVN sums a row's own frames front to back whatever the batch around it (no difference was seen on an MI355X for
    any feature type, route, normalisation or delta setting, so equality is what is asserted)."""
    x = _batch(1e30)
    for normalize, delta in ((True, True), (False, False)):
        fe = _frontend(feat, route, normalize, delta)
        y, _ = fe(x, _lens_dev())
        for b, (n_s, n_f) in enumerate(zip(LENS, NFS)):
            alone = fe(x[b:b + 1, :n_s].contiguous())
            assert alone.shape == (1, fe.feat_dim, n_f)
            assert torch.equal(y[b:b + 1, :, :n_f], alone), (feat, route, normalize, b)


# ------------------------------------------------------------------------------------------ 4. full lengths change nothing
@pytest.mark.parametrize("route", ROUTES)
def test_full_lengths_equal_the_rectangular_call_bit_for_bit(route):
    x = torch.from_numpy(_signals().copy()).to(DEV)
    for feat in FEATS:
        for normalize, delta in ((True, True), (True, False), (False, False)):
            fe = _frontend(feat, route, normalize, delta)
            rect = fe(x)
            assert isinstance(rect, torch.Tensor)                                     # lengths=None: today's return value
            y, nf = fe(x, [S] * len(LENS))
            y2, _ = fe(x, _lens_dev([S] * len(LENS)))
            assert nf.tolist() == [max(NFS)] * len(LENS)
            assert torch.equal(y, rect) and torch.equal(y2, rect), (feat, route, normalize, delta)


def test_device_lengths_are_clamped_and_wrong_dtypes_refused():
    fe = _frontend("mfcc", "fft64")
    x = _batch()
    y, nf = fe(x, _lens_dev([10 ** 6, 1999, 0, -5, 123]))
    assert nf.tolist() == [12, 11, 1, 1, 1]
    want, _ = fe(x, [S, 1999, 1, 1, 123])
    assert torch.equal(y, want)
    with pytest.raises(TypeError):
        fe(x, torch.tensor(LENS, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        fe(x, _lens_dev(LENS[:3]))


# ------------------------------------------------------------------------------------------ 5. one recorded plan, new lengths
def _wave_batch(lens, S_pad, key):
    x = np.zeros((len(lens), S_pad), dtype=np.float32)
    t = np.arange(S_pad) / 16000.0
    for b, n in enumerate(lens):
        x[b, :n] = (0.3 * np.sin(2 * np.pi * (180 + 90 * b) * t) + 0.05 * wg.gen(f"{key}.{b}", (S_pad,)))[:n]
    return torch.from_numpy(x).to(DEV)


def test_a_recorded_plan_follows_the_lengths_in_its_buffer():
    """Front-end + E-TDNN extraction recorded once for [3, 6640] (40 frames); the replay on other waves and other lengths equals
    the eager call on them, and each of its rows the utterance run alone (tests/test_ragged_gpu.py's 1e-6 bar)."""
    from deeplip_amd import packing
    from deeplip_amd.plan import StepPlan
    from models.audio_models.tdnn import SpeakerEmbNet
    packing.set_precision("f16x3")
    try:
        net, _ = load(SpeakerEmbNet(etdnn_opts(24)), "fe.rag.plan.")
        fe = _frontend("mfcc", "fft64")
        S_pad = 400 + 39 * 160

        def step(wave, lens):
            feats, nf = fe(wave, lens)
            return net.extract_embedding(feats, lengths=nf)[0]

        l0, l1 = [6640, 5000, 4100], [4000, 6640, 6333]                              # 40 30 25 frames, then 24 40 39
        ins0 = (_wave_batch(l0, S_pad, "fe.rag.p0"), _lens_dev(l0))
        plan = StepPlan(step, *ins0)
        first = plan.run().clone()
        torch.cuda.synchronize()
        assert torch.equal(first, step(*ins0))
        ins1 = (_wave_batch(l1, S_pad, "fe.rag.p1"), _lens_dev(l1))
        got = plan(*ins1).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, step(*ins1)) and not torch.equal(got, first)
        for b, n in enumerate(l1):
            alone = net.extract_embedding(fe(ins1[0][b:b + 1, :n].contiguous()))[0]
            assert rel_err(got[b:b + 1].cpu().numpy(), alone.cpu().numpy()) < 1e-6, b
        plan.close()
    finally:
        packing.set_precision("f32")


# ------------------------------------------------------------------------------------------ 6. extraction from waveforms
def _resnet():
    from models.resnet import SpeakerEmbNet
    return SpeakerEmbNet({"arch": "resnet", "resnet": {"input_dim": 1, "hidden_dim": [32, 64], "residual_block_layers": [1, 1], "fc_layers": 1,
                                                       "embedding_dim": 64, "pooling": "average"}})


@pytest.mark.parametrize("arch", ["etdnn", "resnet"])
def test_extraction_from_waveforms_equals_one_utterance_at_a_time(arch):
    """24 utterances of 24 .. 60 frames through RaggedExtractor.run(waves=True) == each utterance's waveform through the front-end
    alone and its features through the encoder alone (the bar of tests/test_ragged_gpu.py's own batched-vs-alone comparison: 1e-6),
    in list order; a second pass records nothing."""
    from deeplip_amd import packing
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.synthetic import SyntheticAVSet
    packing.set_precision("f16x3")
    try:
        if arch == "etdnn":
            from models.audio_models.tdnn import SpeakerEmbNet
            net, _ = load(SpeakerEmbNet(etdnn_opts(24)), "fe.rag.ex.")
            fe, D, min_frames = _frontend("mfcc", "fft64"), 512, net.frames_consumed() + 2
        else:
            net, _ = load(_resnet(), "fe.rag.exr.")
            fe, D, min_frames = _frontend("logfbank", "fft64"), 64, 1
        ds = SyntheticAVSet(4, 6, 0, key="fe.rag.ex", ragged=True, audio_range=(24, 60))
        assert len(ds) == 24 and int(ds.audio_len.min()) >= min_frames

        def audio_fn(wave, sample_len):
            feats, nf = fe(wave, sample_len)
            return net.extract_embedding(feats, lengths=nf)[0]

        ex = RaggedExtractor(audio_fn, None, torch.device(DEV), batch=4, waste=0.10, audio_min_frames=min_frames,
                             wave_geometry=(fe.frame_len, fe.frame_step))
        xa, xv = ex.run(ds, 0, len(ds), D, waves=True)
        st = dict(ex.stats)
        xa2, _ = ex.run(ds, 0, len(ds), D, waves=True)
        assert xv is None and ex.stats["plans_recorded"] == st["plans_recorded"] == st["audio_shapes"] >= 3
        assert st["valid_audio_frames"] == int(ds.audio_len.sum()) and torch.equal(xa, xa2)
        ex.close()
        for i in range(len(ds)):
            w = torch.from_numpy(ds.wave_item(i)[None]).to(DEV)
            want = net.extract_embedding(fe(w))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        packing.set_precision("f32")


# ------------------------------------------------------------------------------------------ 7. the entry point
SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
         "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
         "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False}


RESNET = {"model.audio_config.arch": "resnet", "data.python_data_config.feat_dim": 26, "data.python_data_config.feat_type": "fbank",
          "model.audio_config.resnet": {"input_dim": 1, "hidden_dim": [32, 64], "residual_block_layers": [1, 1], "fc_layers": 1,
                                        "embedding_dim": 512, "pooling": "average"}}


def test_av_test_from_waveforms_with_the_resnet_speech_encoder(tmp_path, monkeypatch):
    """The same switch with ``arch: resnet`` (fbank-26 front-end, [B,1,F,T] encoder, minimum length one frame)."""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("av_test", overrides=dict(SMALL, **RESNET, **{"data.python_data_config.test_from_waves": True}))
    try:
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        st = tr.extract_stats
        assert st["plans_recorded"] <= st["audio_shapes"] + st["video_shapes"]
        eer, _ = tr.eer_cos(ds, tr.lomgrid_tables, "cos")
        assert np.isfinite(eer) and 0.0 <= eer <= 1.0
        fe = tr._test_frontend("resnet")
        assert fe.feat_type == "fbank" and fe.feat_dim == 26
        xa = tr.lomgrid_tables[1].emb
        for i in range(len(ds)):
            want = tr.model_audio.extract_embedding(fe(torch.from_numpy(ds.wave_item(i)[None]).to(tr.device)))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        tr.close()


def test_av_test_from_waveforms(tmp_path, monkeypatch):
    """train_fusion's av_test with data.python_data_config.test_from_waves: the speech rows are front-end + encoder of each
    utterance's waveform (checked one at a time), the EER is finite, one plan per bucket shape.  Switch off: the speech rows are the
    encoder on the set's FEATURES one utterance at a time -- what the flow computed before the switch existed (and what
    tests/test_train_fusion_gpu.py pins to the oracle's loop)."""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("av_test", overrides=dict(SMALL, **{"data.python_data_config.test_from_waves": True}))
    try:
        assert tr.test_from_waves
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        st = tr.extract_stats
        assert st["plans_recorded"] <= st["audio_shapes"] + st["video_shapes"] and st["valid_audio_frames"] == int(ds.audio_len.sum())
        eer, _ = tr.eer_cos(ds, tr.lomgrid_tables, "cos")
        assert np.isfinite(eer) and 0.0 <= eer <= 1.0
        fe = tr._test_frontend("etdnn")
        xa = tr.lomgrid_tables[1].emb
        assert torch.isfinite(tr.lomgrid_tables[0].emb).all()
        for i in range(len(ds)):
            want = tr.model_audio.extract_embedding(fe(torch.from_numpy(ds.wave_item(i)[None]).to(tr.device)))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        tr.close()
    off = train_fusion.Trainer("av_test", overrides=dict(SMALL))
    try:
        assert not off.test_from_waves
        off.extract_test_xv_lomgrid()
        xa_off = off.lomgrid_tables[1].emb
        for i in range(len(ds)):
            want = off.model_audio.extract_embedding(torch.from_numpy(off.lomgridtestset.audio_item(i)[None]).to(off.device))[0]
            assert rel_err(xa_off[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
        assert not torch.equal(xa_off, xa)
    finally:
        off.close()
