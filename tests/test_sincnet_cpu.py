"""``arch: sincnet`` without a GPU: the fp64 yardstick against a plain conv1d formulation, the taps' properties, the frame
counts, the config parsing and its refusals, the state-dict schema, and the new entry points in header / binding / library."""
import numpy as np
import pytest
import torch

import sinc_ref as ref

GEOMS = [(25, 10), (400, 160)]


def _taps(F_=6, L=31, rate=16000, grad=False):
    low, band = (torch.from_numpy(v).double() for v in ref.mel_edges(F_, rate))
    if grad:
        low.requires_grad_(), band.requires_grad_()
    return low, band, ref.taps(low, band, L, rate)


@pytest.mark.parametrize("L", [3, 31, 251])
@pytest.mark.parametrize("flen,step", GEOMS)
def test_reference_agrees_with_plain_conv1d(L, flen, step):
    """The term-by-term restatement and conv1d / square / unfold / log are the same function of a rectangular batch, in fp64."""
    _, _, g = _taps(5, L)
    x = ref.white_noise(2, flen + 2 * step + 7, seed=L)
    a, b = ref.features(x, None, g, flen, step), ref.features_conv1d(x, g, flen, step)
    assert a.shape == b.shape == (2, 5, ref.num_frames(x.shape[1], flen, step))
    assert float((a - b).abs().max()) < 1e-12 * float(b.abs().max())


def test_ragged_rows_of_the_reference_are_the_rows_alone():
    _, _, g = _taps(4, 31)
    x = ref.white_noise(3, 1000, seed=2)
    lens = [407, 1000, 399]
    y = ref.features(x, lens, g, 400, 160)
    for b, n in enumerate(lens):
        alone = ref.features(x[b:b + 1, :n], None, g, 400, 160)
        nf = ref.num_frames(n, 400, 160)
        assert alone.shape[2] == nf and torch.equal(y[b, :, :nf], alone[0]) and not y[b, :, nf:].any()


def test_white_noise_band_energies_sit_far_above_eps():
    """What the GPU tests rely on: with unit-variance noise every band energy is orders above eps = 1e-6, so log() does not amplify
    the rounding of e."""
    for L in (3, 31, 251):
        _, _, g = _taps(24, L)
        y = ref.features(ref.white_noise(1, 2000, seed=1), None, g, 400, 160, eps=1e-6)
        assert float(y.min()) > np.log(1e-4), (L, float(y.min()))


def test_taps_are_even_with_a_unit_centre():
    for L in (3, 31, 251, 1023):
        _, _, g = _taps(7, L)
        assert g.shape == (7, L) and torch.equal(g, g.flip(1)) and torch.equal(g[:, (L - 1) // 2], torch.ones(7, dtype=torch.float64))
    # the formula at m and -m, written out: the same value (sin is odd, the Hamming window symmetric)
    low, band, g = _taps(3, 9)
    f1 = 50.0 + low.abs()
    f2 = f1 + 50.0 + band.abs()
    for f in range(3):
        for l in range(9):
            m = l - 4
            if m:
                w = 0.54 - 0.46 * np.cos(2 * np.pi * l / 8)
                v = w * (np.sin(2 * np.pi * float(f2[f]) * m / 16000) - np.sin(2 * np.pi * float(f1[f]) * m / 16000)) / \
                    ((np.pi * m / 16000) * 2 * float(f2[f] - f1[f]))
                assert abs(float(g[f, l]) - v) < 1e-12 * max(1.0, abs(v))


def test_a_clamped_upper_edge_has_zero_gradient():
    low = torch.tensor([100.0, 7000.0], dtype=torch.float64, requires_grad=True)
    band = torch.tensor([200.0, 3000.0], dtype=torch.float64, requires_grad=True)       # filter 1: f2 = 50 + 7000 + 50 + 3000 > 8000
    g = ref.taps(low, band, 31, 16000)
    g.square().sum().backward()
    assert float(band.grad[1]) == 0.0 and float(band.grad[0]) != 0.0 and float(low.grad[1]) != 0.0


def test_frame_counts_are_num_frames():
    from deeplip_amd.frontend import num_frames
    from deeplip_amd.sincnet import SincConv
    sinc = SincConv(4, kernel_size=31)
    assert (sinc.frame_len, sinc.frame_step) == (400, 160)
    for n in (1, 399, 400, 401, 727, 16000):
        assert sinc.frames_for_samples(n) == num_frames(n, 400, 160) == ref.num_frames(n, 400, 160)
    for T in (1, 2, 99):
        S = sinc.samples_for_frames(T)
        assert sinc.frames_for_samples(S) == T and sinc.frames_for_samples(S + 1) == T + 1
    odd = SincConv(4, kernel_size=31, rate=22050)           # rounded half up, as AudioFrontend rounds them
    assert (odd.frame_len, odd.frame_step) == (551, 221)


def _cfg(**sinc):
    sec = {"input_dim": 24, "hidden_dim": [32, 64], "context": [[-2, -1, 0, 1, 2], [0]], "tdnn_layers": 2, "fc_layers": 3,
           "embedding_dim": 16, "pooling": "statistic", "bn_first": True}
    if sinc:
        sec["sinc"] = dict(sinc)
    return {"arch": "sincnet", "sincnet": sec}


def test_build_speech_encoder_and_the_state_dict():
    from deeplip_amd import trainer_common as tc
    from deeplip_amd.sincnet import SincConv
    m = tc.build_speech_encoder(_cfg(kernel_size=31), wave_cfg={"rate": 8000, "win_len": 0.02})
    assert isinstance(m.sinc, SincConv) and m.sinc.kernel_size == 31 and m.sinc.rate == 8000 and (m.sinc.frame_len, m.sinc.frame_step) == (160, 80)
    sd = m.state_dict()
    assert [k for k in sd if k.startswith("sinc.")] == ["sinc.low_hz_", "sinc.band_hz_"]
    assert tuple(sd["sinc.low_hz_"].shape) == tuple(sd["sinc.band_hz_"].shape) == (24, 1) and sd["sinc.low_hz_"].dtype == torch.float32
    plain = tc.build_speech_encoder({"arch": "tdnn", "tdnn": dict(_cfg()["sincnet"])})
    assert sorted(k for k in sd if not k.startswith("sinc.")) == sorted(plain.state_dict()) and plain.sinc is None
    # the initial values: mel-spaced edges between 30 Hz and rate / 2 - 100
    low, band = ref.mel_edges(24, 8000)
    assert np.allclose(sd["sinc.low_hz_"].view(-1).numpy(), low, rtol=1e-6) and np.allclose(sd["sinc.band_hz_"].view(-1).numpy(), band, rtol=1e-6)
    assert abs(low[0] - 30.0) < 1e-9 and abs(low[-1] + band[-1] - 3900.0) < 1e-6
    d = tc.build_speech_encoder(_cfg())
    assert d.sinc.kernel_size == 251 and d.sinc.rate == 16000 and d.sinc.eps == 1e-6 and d.sinc.min_low_hz == d.sinc.min_band_hz == 50.0
    assert tc.encoder_min_frames(d) == 6


def test_a_feature_tensor_is_refused():
    from deeplip_amd import trainer_common as tc
    m = tc.build_speech_encoder(_cfg(kernel_size=31))
    with pytest.raises(ValueError, match="takes waveforms"):          # (train mode: refused before anything reaches the library)
        m.train().extract_embedding(torch.zeros(2, 24, 50))


@pytest.mark.parametrize("bad", [{"kernel_size": 250}, {"kernel_size": 1}, {"kernel_size": 1025}, {"kernel_size": 31.0}, {"eps": 0.0},
                                 {"min_low_hz": -1.0}, {"taps": 31}])
def test_config_parsing_refuses(bad):
    from deeplip_amd import trainer_common as tc
    with pytest.raises(ValueError, match="sinc"):
        tc.build_speech_encoder(_cfg(**bad))


def test_unknown_architectures_stay_unimplemented():
    from deeplip_amd import trainer_common as tc
    with pytest.raises(NotImplementedError, match="Other models are not implemented"):
        tc.build_speech_encoder({"arch": "rawnet", "rawnet": dict(_cfg()["sincnet"])})


def _sinc_ov():
    return {"model.arch": "sincnet", "model.sincnet": _cfg(kernel_size=31)["sincnet"]}


@pytest.mark.parametrize("extra,msg", [({}, "train_from_waves"), ({"data.train_from_waves": False}, "train_from_waves"),
                                       ({"data.train_from_waves": True, "data.spec_augment": {"freq_masks": 1, "freq_width": 2, "time_masks": 0}},
                                        "spec_augment"),
                                       ({"data.train_from_waves": True, "model.sincnet.sinc.kernel_size": 32}, "kernel_size")])
def test_trainer_refusals_come_before_the_gpu(extra, msg):
    """train_audio.Trainer checks the section on the host: every refusal is a ValueError, raised before the GPU requirement."""
    import train_audio
    with pytest.raises(ValueError, match=msg):
        train_audio.Trainer(overrides={**_sinc_ov(), **extra})


def test_shipped_config_documents_the_section():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "conf", "audio_config.yaml")).read()
    assert "sincnet:" in text and "kernel_size" in text


ARITY = {"dlip_sinc_taps_f32": 9, "dlip_sinc_taps_bwd_f32": 11, "dlip_sinc_features_f32": 16, "dlip_sinc_features_bwd_workspace_bytes": 6,
         "dlip_sinc_features_bwd_f32": 18}


def test_entry_points_in_header_binding_and_library():
    from deeplip_amd import _lib
    l = _lib.lib()
    for n, k in ARITY.items():
        assert len(_lib.SIGNATURES[n]) == k and hasattr(l, n), n
    assert _lib.HEADER["DLIP_SINC_MAX_TAPS"] == 1023 and _lib.HEADER["DLIP_SINC_LDS_SAMPLES"] == 4096


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from deeplip_amd import _lib
    l = _lib.lib()
    P = 4096
    ok = dict(wave=P, lengths=None, g=P, y=P, nf=None, B=2, S=1000, F=24, L=31, flen=400, step=160, NF=5, layout=0, Fp=24, eps=1e-6, stream=None)
    # (only refusals are called: each returns before any launch, so nothing here touches a device)
    for over in (dict(L=32), dict(L=1025), dict(NF=4), dict(layout=1, Fp=23), dict(layout=0, Fp=32), dict(layout=2), dict(eps=0.0), dict(B=0),
                 dict(F=0), dict(wave=None), dict(flen=4067, NF=1), dict(step=0), dict(wave=P + 2)):
        assert l.dlip_sinc_features_f32(*{**ok, **over}.values()) == -1, over
    assert l.dlip_sinc_features_bwd_workspace_bytes(2, 1000, 24, 31, 400, 160) == 2 * 1 * 24 * 16 * 4
    assert l.dlip_sinc_features_bwd_workspace_bytes(2, 1000, 24, 30, 400, 160) < 0
    okb = dict(wave=P, lengths=None, g=P, y=P, dy=P, dg=P, ws=P, nbytes=1 << 20, B=2, S=1000, F=24, L=31, flen=400, step=160, NF=5, layout=1,
               Fp=32, stream=None)
    for over in (dict(nbytes=16), dict(ws=None), dict(ws=P + 4), dict(dy=None), dict(Fp=56), dict(NF=6)):
        assert l.dlip_sinc_features_bwd_f32(*{**okb, **over}.values()) == -1, over
    for bad in ((P, P, P, 24, 30, 16000.0, 50.0, 50.0, None), (P, P, P, 24, 31, 0.0, 50.0, 50.0, None), (None, P, P, 24, 31, 16000.0, 50.0, 50.0, None),
                (P, P, P, 24, 31, 16000.0, -1.0, 50.0, None)):
        assert l.dlip_sinc_taps_f32(*bad) == -1, bad
    assert l.dlip_sinc_taps_bwd_f32(P, P, P, P, None, 24, 31, 16000.0, 50.0, 50.0, None) == -1
