"""The ``stft`` feature type on the GPU (-m gpu): AudioFrontend("stft") against the fp64 restatement of the loaders' definition
(tests/test_stft_cpu.py: librosa.stft -> magphase -> log1p, models/audio_models/datasets.py:72-76; checked there against torch.stft
in fp64), on ragged batches, inside a recorded plan and through RaggedExtractor, train_audio and train_fusion.

Bars.  Un-normalised: |got - ref| <= 1e-9 + 2.5e-7 |ref| for EVERY element -- four times the half-ulp of the one rounding to fp32
that an fp64 pipeline has (2^-24 = 6e-8); window, FFT, modulus and log1p round at 1e-15 and below.  Normalised (with and without
deltas): rel_err < 1e-4, the front-end's bar in tests/test_frontend.py, on noise signals at every geometry.  The noise rows are those
of tests/test_stft_cpu.py's NORM_SEEDS: every bin's deviation over time is healthy there (min over bins of std / |mean| > 0.05,
asserted on the restatement there and here), so the bar is not spent on the cancellation in x - mean; at two and three frames such
rows are rare and their seeds were searched for, as that table says."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_models_gpu import DEV, load
from test_stft_cpu import noise, norm_signals, stft_features_ref, stft_logmag_ref

pytestmark = pytest.mark.gpu

# (n_fft, hop, win, S): the minimum width and the frame-count steps at hop 40 | a window that fills the frame | an odd window centred
# in a padded frame | the shipped geometry, 32 frames
CASES = ((128, 40, 100, 65), (128, 40, 100, 79), (128, 40, 100, 80), (128, 40, 100, 257), (256, 64, 256, 129), (256, 64, 256, 1000),
         (1024, 220, 551, 3000), (512, 160, 400, 5040))
RATE = 1000


def _frontend(n_fft, hop, win, normalize=False, delta=False):
    """(hop + 0.5) / RATE seconds truncates to hop samples whatever the product's last bit is."""
    from deeplip_amd.frontend import AudioFrontend
    fe = AudioFrontend("stft", rate=RATE, win_len=(win + 0.5) / RATE, win_shift=(hop + 0.5) / RATE, nfft=n_fft, normalize=normalize,
                       delta=delta, num_bin=7, num_cep=5, preemph=0.5, ceplifter=3, energy=False)          # (ignored by stft)
    assert (fe.hop, fe.win_length, fe.nfft) == (hop, win, n_fft)
    return fe


@functools.lru_cache(maxsize=None)
def _signals(n_fft, S):
    """[6, S] float32: noise | unit impulse at sample 0 | at sample S - 1 (both reflections) | a constant (every frame's DC bin) |
    a sine on the exact bin centre n_fft / 8 | more noise."""
    x = np.zeros((6, S), dtype=np.float32)
    x[0] = noise(f"stft.gpu.a.{n_fft}.{S}", S)
    x[1, 0] = 1.0
    x[2, S - 1] = 1.0
    x[3] = 0.25
    x[4] = 0.5 * np.sin(2.0 * np.pi * (n_fft // 8) * np.arange(S) / n_fft)
    x[5] = noise(f"stft.gpu.b.{n_fft}.{S}", S)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True)).to(DEV)


# ------------------------------------------------------------------------------------------ 1. parity with the definition
@pytest.mark.parametrize("n_fft,hop,win,S", CASES)
def test_unnormalised_rows_equal_the_fp64_definition_to_one_fp32_rounding(n_fft, hop, win, S):
    fe = _frontend(n_fft, hop, win)
    sig = _signals(n_fft, S)
    T, F = 1 + S // hop, n_fft // 2 + 1
    worst = 0.0
    for rows in (slice(0, 4), slice(4, 6)):                                   # B = 4 and B = 2
        y = fe(_dev(sig[rows]))
        assert isinstance(y, torch.Tensor) and y.shape == (rows.stop - rows.start, F, T) and y.dtype == torch.float32
        y = y.cpu().numpy().astype(np.float64)
        for i, b in enumerate(range(rows.start, rows.stop)):
            ref = stft_logmag_ref(sig[b], n_fft, hop, win).T                  # [F, T]
            excess = np.abs(y[i] - ref) - (1e-9 + 2.5e-7 * np.abs(ref))
            worst = max(worst, float((np.abs(y[i] - ref) / (1e-9 + 2.5e-7 * np.abs(ref))).max()))
            assert (excess <= 0).all(), (b, float(excess.max()), np.unravel_index(int(excess.argmax()), excess.shape))
    print(f"({n_fft}, {hop}, {win}, {S}): largest |err| / (1e-9 + 2.5e-7 |ref|) = {worst:.3f}")
    assert stft_logmag_ref(sig[3], n_fft, hop, win)[:, 0].min() > 1.0         # the constant: every frame's DC bin, edge frames included


@pytest.mark.parametrize("n_fft,hop,win,S", CASES)
def test_normalised_features_and_deltas_equal_the_definition(n_fft, hop, win, S):
    sig = norm_signals(n_fft, hop, win, S)
    B = len(sig)
    for b in range(B):
        raw = stft_logmag_ref(sig[b], n_fft, hop, win)
        assert float((raw.std(axis=0) / np.abs(raw.mean(axis=0))).min()) > 0.05, b        # healthy bins: see the module docstring
    for delta in (False, True):
        fe = _frontend(n_fft, hop, win, normalize=True, delta=delta)
        y = fe(_dev(sig)).cpu().numpy()
        assert y.shape == (B, fe.feat_dim, 1 + S // hop) and fe.feat_dim == (3 if delta else 1) * (n_fft // 2 + 1)
        for b in range(B):
            e = rel_err(y[b], stft_features_ref(sig[b], n_fft, hop, win, normalize=True, delta=delta))
            print(f"({n_fft}, {hop}, {win}, {S}) delta={delta} row {b}: rel_err {e:.3e}")
            assert e < 1e-4, (delta, b)


# ------------------------------------------------------------------------------------------ 2. ragged batches
LENS, S_PAD, RAG = (65, 79, 80, 257), 300, (128, 40, 100)
NFS = tuple(1 + n // RAG[1] for n in LENS)


def _ragged_batch(fill):
    x = np.full((len(LENS), S_PAD), fill, dtype=np.float32)
    for b, n in enumerate(LENS):
        x[b, :n] = noise(f"stft.rag.{b}", S_PAD)[:n]
    return _dev(x)


def _lens_dev(vals=LENS):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("normalize,delta", [(False, False), (True, False), (True, True)])
def test_each_ragged_row_is_the_row_alone_bit_for_bit(normalize, delta):
    fe = _frontend(*RAG, normalize=normalize, delta=delta)
    x = _ragged_batch(float("nan"))                                           # NaN in every padded sample: none is read
    y, nf = fe(x, list(LENS))
    assert nf.dtype == torch.int32 and nf.is_cuda and nf.tolist() == list(NFS) == [2, 2, 3, 7]
    assert y.shape == (len(LENS), fe.feat_dim, 1 + S_PAD // RAG[1]) and torch.isfinite(y).all()
    for b, (n, t) in enumerate(zip(LENS, NFS)):
        alone = fe(x[b:b + 1, :n].contiguous())
        assert alone.shape == (1, fe.feat_dim, t)
        assert torch.equal(y[b:b + 1, :, :t], alone), b
        assert not y[b, :, t:].any(), b                                       # exact zeros past the row's frames
        assert y[b, :, :t].any()
    y2, nf2 = fe(x, _lens_dev())                                              # a device vector: the same bits as the host list
    assert torch.equal(nf2, nf) and torch.equal(y2, y)
    if not normalize:                                                         # ... and the definition, row by row
        for b, (n, t) in enumerate(zip(LENS, NFS)):
            ref = stft_logmag_ref(x[b, :n].cpu().numpy(), *RAG).T
            assert (np.abs(y[b, :, :t].cpu().numpy() - ref) <= 1e-9 + 2.5e-7 * np.abs(ref)).all(), b


def test_device_lengths_are_clamped_and_host_lengths_validated():
    fe = _frontend(*RAG, normalize=True)
    x = _ragged_batch(0.0)
    y, nf = fe(x, _lens_dev([10, 79, 0, 10 ** 6]))                            # below the minimum -> 65, above the width -> 300
    assert nf.tolist() == [2, 2, 2, 8]
    want, nfw = fe(x, [65, 79, 65, S_PAD])
    assert torch.equal(y, want) and torch.equal(nf, nfw) and torch.isfinite(y).all()
    full, nff = fe(x, [S_PAD] * 4)                                            # full lengths: the rectangular call's bits
    assert torch.equal(full, fe(x)) and nff.tolist() == [8] * 4
    for bad in ([64, 79, 80, 257], [65, 79, 80, S_PAD + 1], [65, 79, 80]):
        with pytest.raises(ValueError):
            fe(x, bad)
    with pytest.raises(TypeError):
        fe(x, torch.tensor(LENS, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        fe(x[:, :64].contiguous())                                            # narrower than nfft // 2 + 1


# ------------------------------------------------------------------------------------------ 3. a recorded plan
def test_the_call_records_into_a_step_plan():
    """Recorded once; the replay equals the eager call bit for bit, on the recorded inputs and on other waves and lengths."""
    from deeplip_amd.plan import StepPlan
    fe = _frontend(*RAG, normalize=True, delta=True)

    def step(wave, lens):
        feats, nf = fe(wave, lens)
        return feats

    ins0 = (_ragged_batch(0.0), _lens_dev())
    plan = StepPlan(step, *ins0)
    first = plan.run().clone()
    torch.cuda.synchronize()
    assert torch.equal(first, step(*ins0))
    l1 = [257, 65, 300, 141]
    x1 = _dev(np.stack([noise(f"stft.plan.{b}", S_PAD) for b in range(4)]))
    got = plan(x1, _lens_dev(l1)).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, step(x1, _lens_dev(l1))) and not torch.equal(got, first)
    plan.close()
    rect = StepPlan(lambda wave: fe(wave), ins0[0])
    out = rect.run().clone()
    torch.cuda.synchronize()
    assert torch.equal(out, fe(ins0[0]))
    rect.close()


# ------------------------------------------------------------------------------------------ 4. through the callers
RESNET_OPTS = {"input_dim": 1, "hidden_dim": [16, 32], "residual_block_layers": [1, 1], "fc_layers": 1, "embedding_dim": 64,
               "pooling": "average"}
WAVE_GEOM = {"rate": 4000, "nfft": 128, "feat_type": "stft", "feat_dim": 65}           # 25 ms / 10 ms: window 100, hop 40, 65 bins


def test_extraction_from_waveforms_equals_one_utterance_at_a_time():
    """RaggedExtractor.run(waves=True) with the stft front-end as its geometry and the `arch: resnet` encoder == each utterance's
    waveform through front-end and encoder alone (1e-6, the bar of tests/test_frontend_ragged_gpu.py's extraction test)."""
    from deeplip_amd import packing
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.frontend import AudioFrontend
    from deeplip_amd.synthetic import SyntheticAVSet
    from models.resnet import SpeakerEmbNet
    packing.set_precision("f16x3")
    try:
        net, _ = load(SpeakerEmbNet({"arch": "resnet", "resnet": dict(RESNET_OPTS)}), "stft.ex.")
        fe = AudioFrontend("stft", rate=4000, nfft=128)
        assert (fe.frame_len, fe.frame_step, fe.feat_dim) == (100, 40, 65)
        ds = SyntheticAVSet(3, 4, 0, key="stft.ex", ragged=True, audio_range=(24, 60))

        def audio_fn(wave, sample_len):
            feats, nf = fe(wave, sample_len)
            return net.extract_embedding(feats, lengths=nf)[0]

        ex = RaggedExtractor(audio_fn, None, torch.device(DEV), batch=4, waste=0.10, wave_geometry=fe)
        xa, xv = ex.run(ds, 0, len(ds), 64, waves=True)
        st = dict(ex.stats)
        slen = ds.wave_len(100, 40)
        assert xv is None and st["plans_recorded"] == st["audio_shapes"] >= 1
        assert st["valid_audio_frames"] == int(sum(1 + int(s) // 40 for s in slen))     # the front-end's own frame count
        ex.close()
        for i in range(len(ds)):
            w = torch.from_numpy(ds.wave_item(i, 100, 40)[None]).to(DEV)
            assert w.shape[1] == int(slen[i])
            want = net.extract_embedding(fe(w))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        packing.set_precision("f32")


def test_train_audio_from_waves_with_spectrogram_features(tmp_path, monkeypatch):
    """Two recorded steps of train_audio.Trainer on stft features: a crop of T frames is cut as window + (T - 1) hop samples, as the
    loader's collate cuts it (datasets.py:113-115), and the encoder sees the T + 2 spectrogram frames librosa.stft makes of them."""
    import train_audio
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    ov = {"model.arch": "resnet", "data.feat_type": "stft", "data.feat_dim": 65, "data.nfft": 128, "data.rate": 4000,
          "data.train_from_waves": True, "model.resnet.hidden_dim": [16, 32], "model.resnet.residual_block_layers": [1, 1],
          "model.resnet.embedding_dim": 32, "data.n_spk": 5, "data.utt_per_spk": 2, "data.test_speakers": 2, "data.test_utt_per_spk": 2,
          "data.audio_frames": 60, "train.bs": 4, "train.steps_per_epoch": 2, "train.crop_frames": [40, 40]}
    tr = train_audio.Trainer(overrides=ov)
    try:
        assert tr._wave_fe.feat_type == "stft" and tr._wave_fe.feat_dim == 65 and (tr._wave_fe.frame_len, tr._wave_fe.frame_step) == (100, 40)
        seen = []
        one_step = tr._one_step
        monkeypatch.setattr(tr, "_one_step", lambda x, lab: (seen.append(tuple(x.shape)), one_step(x, lab))[1])
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        st = tr.last_epoch_stats
        assert np.isfinite(loss) and np.isfinite(st["loss"]) and st["from_waves"] is True and st["steps"] == 2
        assert st["crop_ladder"] == [40] and st["step_mode"] in ("eager (warm-up)", "graph")
        assert seen and all(s == (4, 65, 42) for s in seen), seen             # 100 + 39 * 40 = 1660 samples -> 1 + 1660 // 40 = 42
    finally:
        tr.close()
    with pytest.raises(ValueError, match="front-end yields 65"):
        train_audio.Trainer(overrides=dict(ov, **{"data.feat_dim": 64}))


def test_av_test_from_waveforms_with_spectrogram_features(tmp_path, monkeypatch):
    import train_fusion
    monkeypatch.chdir(tmp_path)
    small = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
             "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
             "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False,
             "model.audio_config.arch": "resnet", "model.audio_config.resnet": dict(RESNET_OPTS, embedding_dim=512),
             "data.python_data_config.test_from_waves": True}
    small.update({f"data.python_data_config.{k}": v for k, v in WAVE_GEOM.items()})
    tr = train_fusion.Trainer("av_test", overrides=small)
    try:
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        st = tr.extract_stats
        assert st["plans_recorded"] <= st["audio_shapes"] + st["video_shapes"]
        eer, _ = tr.eer_cos(ds, tr.lomgrid_tables, "cos")
        assert np.isfinite(eer) and 0.0 <= eer <= 1.0
        fe = tr._test_frontend("resnet")
        assert fe.feat_type == "stft" and fe.feat_dim == 65 and tr._ragged_extractor(4).wave_frontend is not None
        xa = tr.lomgrid_tables[1].emb
        for i in range(0, len(ds), 3):
            want = tr.model_audio.extract_embedding(fe(torch.from_numpy(ds.wave_item(i, 100, 40)[None]).to(tr.device)))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        tr.close()
