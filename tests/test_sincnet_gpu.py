"""``arch: sincnet`` on the GPU (-m gpu) against tests/sinc_ref.py, the fp64 restatement of its definition: the sinc layer's
forward and backward at the tile, chunk and length edges, ragged batches (rows bit-identical to rows run alone, the padding never read),
determinism, the footprint of every launch, the memory the layer allocates, the encoder in eval and train mode under both TRAIN_CONV
modes, the recorded step of train_audio.Trainer and extraction to an EER.

Bars are the project's: 2e-5 of the tensor's largest magnitude on outputs, 1e-4 of each gradient tensor's largest magnitude on
gradients (tests/test_train_f32_gpu.py).  Inputs are unit-variance white noise: every band energy sits orders above eps
(tests/test_sincnet_cpu.py), so the log does not amplify the rounding of the energies."""
import functools
import gc
import re

import numpy as np
import pytest
import torch

import sinc_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_OUT, BAR_GRAD = 2e-5, 1e-4
RATE = 16000
GEOMS = [(25, 10), (400, 160)]


@pytest.fixture(autouse=True)
def _clean_status():
    from deeplip_amd import _lib
    torch.cuda.synchronize()
    _lib.status_words().zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_words().zero_()


def _layer(F_, L, flen=400, step=160, eps=1e-6):
    from deeplip_amd.sincnet import SincConv
    sinc = SincConv(F_, kernel_size=L, eps=eps, rate=RATE, win_len=flen / RATE, win_shift=step / RATE).to(DEV)
    assert (sinc.frame_len, sinc.frame_step) == (flen, step)
    return sinc


def _lengths(flen, step):
    return [flen - 1, flen, flen + 1, flen + 2 * step + 7]


@functools.lru_cache(maxsize=None)
def _case(F_, L, flen, step, long=False):
    """One ragged batch and everything the reference says about it, computed once: y, and for a fixed dy the gradients of the taps
    (symmetrised: the kernel returns the gradient on the even taps) and of the two parameters."""
    lens = [16000] if long else _lengths(flen, step)
    x = ref.white_noise(len(lens), max(lens), seed=F_ + L + flen).float().double()          # (fp32-representable samples)
    low, band = (torch.from_numpy(v).float().double().requires_grad_() for v in ref.mel_edges(F_, RATE))
    g = ref.taps(low, band, L, RATE)
    g.retain_grad()
    y = ref.features(x, lens, g, flen, step)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(L), dtype=torch.float64).float().double()
    (y * dy).sum().backward()
    dg = 0.5 * (g.grad + g.grad.flip(1))
    return dict(lens=lens, x=x.float(), y=y.detach(), dy=dy.float(), dg=dg, dlow=low.grad.view(-1, 1), dband=band.grad.view(-1, 1))


CASES = [(F_, L, flen, step) for L in (3, 31, 251) for F_ in (4, 24, 40) for flen, step in GEOMS]


@pytest.mark.parametrize("F_,L,flen,step", CASES)
def test_forward_against_fp64(F_, L, flen, step):
    _check_forward(F_, L, flen, step, False)


def test_forward_against_fp64_one_second():
    _check_forward(24, 251, 400, 160, True)


def _check_forward(F_, L, flen, step, long):
    c = _case(F_, L, flen, step, long)
    sinc = _layer(F_, L, flen, step)
    x = c["x"].to(DEV)
    with torch.no_grad():
        y, nf = sinc(x, c["lens"])
        Fp = (F_ + 31) // 32 * 32
        yc, nfc = sinc.features(x, c["lens"], channels_last_pad=Fp)
    torch.cuda.synchronize()
    want = c["y"].numpy()
    assert nf.cpu().tolist() == nfc.cpu().tolist() == [ref.num_frames(n, flen, step) for n in c["lens"]]
    e = rel_err(y.cpu().numpy(), want)
    print(f"\nforward F {F_} L {L} ({flen}, {step}) lens {c['lens']}: rel err {e:.3e}")
    assert tuple(y.shape) == want.shape and e < BAR_OUT
    # the channels-last layout holds the same bits, its padding channels zeros
    assert torch.equal(yc[:, :, :F_].permute(0, 2, 1), y) and not yc[:, :, F_:].any()
    # frames at or past a row's count are exactly zero
    for b, n in enumerate(nf.cpu().tolist()):
        assert not y[b, :, n:].any()


@pytest.mark.parametrize("F_,L,flen,step", CASES)
def test_backward_against_fp64_autograd(F_, L, flen, step):
    """dg and the two parameter gradients; with (25, 10) and L = 31 or 251 every row is shorter than the filter."""
    from deeplip_amd.sincnet import SincFeaturesFn
    c = _case(F_, L, flen, step)
    sinc = _layer(F_, L, flen, step)
    x, dy = c["x"].to(DEV), c["dy"].to(DEV)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    g = sinc.taps().detach().requires_grad_()
    y, _ = SincFeaturesFn.apply(g, x, lens, flen, step, 0, sinc.eps)
    y.backward(dy)
    y2, _ = sinc(x, lens)
    y2.backward(dy)
    torch.cuda.synchronize()
    errs = {"dg": rel_err(g.grad.cpu().numpy(), c["dg"].numpy()), "d low_hz_": rel_err(sinc.low_hz_.grad.cpu().numpy(), c["dlow"].numpy()),
            "d band_hz_": rel_err(sinc.band_hz_.grad.cpu().numpy(), c["dband"].numpy())}
    print(f"\nbackward F {F_} L {L} ({flen}, {step}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.equal(g.grad, g.grad.flip(1))
    assert all(v < BAR_GRAD for v in errs.values()), errs
    # the channels-last layout yields the same gradient bits
    Fp = (F_ + 31) // 32 * 32
    g3 = sinc.taps().detach().requires_grad_()
    yc, _ = SincFeaturesFn.apply(g3, x, lens, flen, step, Fp, sinc.eps)
    dyc = torch.full((dy.shape[0], dy.shape[2], Fp), float("nan"), device=DEV)
    dyc[:, :, :F_] = dy.permute(0, 2, 1)
    yc.backward(dyc)
    assert torch.equal(g3.grad, g.grad)


def test_a_clamped_filter_gets_no_band_gradient():
    sinc = _layer(4, 31)
    with torch.no_grad():
        sinc.low_hz_[3] = 7000.0
        sinc.band_hz_[3] = 3000.0
    x = ref.white_noise(2, 1000, seed=3).float().to(DEV)
    y, _ = sinc(x, [1000, 600])
    y.square().sum().backward()
    torch.cuda.synchronize()
    assert float(sinc.band_hz_.grad[3]) == 0.0 and float(sinc.band_hz_.grad[0]) != 0.0 and float(sinc.low_hz_.grad[3]) != 0.0
    assert bool(torch.isfinite(sinc.low_hz_.grad).all())


@pytest.mark.parametrize("L", [31, 251])
def test_ragged_rows_are_the_rows_alone_and_the_padding_is_never_read(L):
    sinc = _layer(24, L)
    lens = [407, 1000, 399]
    x = ref.white_noise(3, 1000, seed=11).float()
    for b, n in enumerate(lens):
        x[b, n:] = 0.0
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan")                       # poisoned padding
    with torch.no_grad():
        y, nf = sinc(x.to(DEV), lens)
        yp, _ = sinc(xp.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
        yc, _ = sinc.features(xp.to(DEV), lens, channels_last_pad=32)
        alone = [sinc(x[b:b + 1, :n].contiguous().to(DEV)) for b, n in enumerate(lens)]
    torch.cuda.synchronize()
    assert torch.equal(y, yp) and bool(torch.isfinite(y).all())
    assert torch.equal(yc[:, :, :24].permute(0, 2, 1), y) and not yc[:, :, 24:].any()
    for b, n in enumerate(nf.cpu().tolist()):
        assert alone[b].shape[2] == n and torch.equal(y[b, :, :n], alone[b][0]), b
        assert not y[b, :, n:].any()


def test_two_backward_runs_have_the_same_bits():
    sinc = _layer(24, 251)
    x = ref.white_noise(6, 4000, seed=5).float().to(DEV)
    lens = [4000, 3999, 2500, 401, 400, 77]
    grads = []
    for _ in range(2):
        sinc.zero_grad(set_to_none=True)
        y, _ = sinc(x, lens)
        y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
        grads.append((sinc.low_hz_.grad.clone(), sinc.band_hz_.grad.clone()))
    torch.cuda.synchronize()
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert bool(torch.isfinite(grads[0][0]).all()) and float(grads[0][0].abs().max()) > 0.0


@pytest.mark.parametrize("F_,L,layout", [(24, 251, 0), (24, 31, 1), (40, 31, 1), (4, 3, 0)])
def test_launches_stay_inside_their_buffers(F_, L, layout):
    """wave, g, y, frame_lengths, dy, dg and the workspace in fenced allocations: the fences stay intact, the outputs are fully written."""
    from footprint import FenceArena
    from deeplip_amd._lib import call, lib
    flen, step = 400, 160
    lens = [1000, 407, 399]
    B, S = 3, 1000
    NF = ref.num_frames(S, flen, step)
    Fp = (F_ + 31) // 32 * 32 if layout else F_
    sinc = _layer(F_, L)
    arena = FenceArena()
    wave = arena.fenced(ref.white_noise(B, S, seed=9).float().to(DEV), "wave")
    lv = arena.fenced(torch.tensor(lens, dtype=torch.int32, device=DEV), "lengths")
    with torch.no_grad():
        g = arena.fenced(sinc.taps(), "g")
    shape = (B, NF, Fp) if layout else (B, F_, NF)
    y = arena.filled(shape, DEV, name="y")
    nf = arena.filled((B,), DEV, torch.int32, name="frame_lengths")
    call("dlip_sinc_features_f32", wave, lv, g, y, nf, B, S, F_, L, flen, step, NF, layout, Fp, 1e-6)
    torch.cuda.synchronize()
    arena.check_all("forward")
    assert not arena.unwritten(y) and not arena.unwritten(nf) and bool(torch.isfinite(y).all())
    dy = arena.fenced(torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(DEV), "dy")
    dg = arena.filled((F_, L), DEV, name="dg")
    nbytes = int(lib().dlip_sinc_features_bwd_workspace_bytes(B, S, F_, L, flen, step))
    ws = arena.filled((nbytes // 4,), DEV, name="workspace")
    call("dlip_sinc_features_bwd_f32", wave, lv, g, y, dy, dg, ws, nbytes, B, S, F_, L, flen, step, NF, layout, Fp)
    dlow, dband = arena.filled((F_, 1), DEV, name="dlow"), arena.filled((F_, 1), DEV, name="dband")
    low, band = arena.fenced(sinc.low_hz_.detach(), "low"), arena.fenced(sinc.band_hz_.detach(), "band")
    call("dlip_sinc_taps_bwd_f32", low, band, dg, dlow, dband, F_, L, float(RATE), 50.0, 50.0)
    g2 = arena.filled((F_, L), DEV, name="g2")
    call("dlip_sinc_taps_f32", low, band, g2, F_, L, float(RATE), 50.0, 50.0)
    torch.cuda.synchronize()
    arena.check_all("backward")
    for t in (dg, ws, dlow, dband, g2):
        assert not arena.unwritten(t) and bool(torch.isfinite(t).all())
    assert torch.equal(g2, g)


def test_no_stride_one_tensor_is_allocated():
    """One forward + backward of the layer at B = 8, S = 16000, F = 24 raises the allocated peak by less than HALF of one stride-1
    intermediate z [B, F, S] (which a torch formulation writes, and keeps for its backward)."""
    B, S, F_ = 8, 16000, 24
    sinc = _layer(F_, 251)
    x = ref.white_noise(B, S, seed=4).float().to(DEV)
    y, _ = sinc.features(x, None)          # warm: kernels loaded, nothing cached that the measurement would count
    y.sum().backward()
    del y
    sinc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y, _ = sinc.features(x, None)
    y.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"\npeak rise of one forward + backward: {rise} bytes; half a stride-1 tensor: {B * F_ * S * 4 // 2}")
    assert rise < B * F_ * S * 4 // 2


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------
CONTEXTS = [[-2, -1, 0, 1, 2], [-1, 0, 1]]
SINC = dict(L=31, rate=RATE, min_low_hz=50.0, min_band_hz=50.0, eps=1e-6, frame_len=400, frame_step=160)


def _cfg():
    return {"arch": "sincnet", "sincnet": {"input_dim": 24, "hidden_dim": [32, 32], "context": CONTEXTS, "tdnn_layers": 2, "fc_layers": 3,
                                           "embedding_dim": 16, "pooling": "statistic", "bn_first": True, "sinc": {"kernel_size": 31}}}


def _encoder():
    from deeplip_amd import trainer_common as tc, weightgen as wg
    m = tc.build_speech_encoder(_cfg())
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("sinc.")}, prefix="audio.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def _waves(B, T, seed):
    return ref.white_noise(B, 400 + (T - 1) * 160, seed=seed).float()


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_encoder_eval_parity_and_ragged_rows(mode):
    import ftdnn_ref
    from deeplip_amd import _lib, arith, trainer_common as tc
    arith.configure(mode)
    m = _encoder().eval().to(DEV)
    assert tc.encoder_min_frames(m) == 8
    x = _waves(3, 20, seed=21)
    with torch.no_grad():
        xv, xa = m.extract_embedding(x.to(DEV))
        p = ftdnn_ref.to64(m.state_dict())
        wv, wa = ref.encoder(x.double(), None, p, CONTEXTS, True, False, SINC)
    _lib.check_range(sync=True)
    ev, ea = rel_err(xv.cpu().numpy(), wv.numpy()), rel_err(xa.cpu().numpy(), wa.numpy())
    print(f"\nencoder eval {mode}: xv {ev:.3e}, x_a {ea:.3e}")
    assert ev < BAR_OUT and ea < BAR_OUT
    lens = [x.shape[1], 400 + 7 * 160, 2001]
    xr = x.clone()
    for b, n in enumerate(lens):
        xr[b, n:] = 0.0
    with torch.no_grad():
        rv, ra = m.extract_embedding(xr.to(DEV), lengths=lens)
        dv, da = m.extract_embedding(xr.to(DEV), lengths=torch.tensor(lens, dtype=torch.int32, device=DEV))
        alone = [m.extract_embedding(xr[b:b + 1, :n].contiguous().to(DEV)) for b, n in enumerate(lens)]
        wr, _ = ref.encoder(xr.double(), lens, p, CONTEXTS, True, False, SINC)
    _lib.check_range(sync=True)
    for b in range(3):
        assert torch.equal(rv[b], alone[b][0][0]) and torch.equal(ra[b], alone[b][1][0]), b
    assert torch.equal(rv, dv) and torch.equal(ra, da) and torch.equal(rv[0], xv[0])
    assert rel_err(rv.cpu().numpy(), wr.numpy()) < BAR_OUT
    with pytest.raises(ValueError, match="takes waveforms"):
        m.extract_embedding(torch.zeros(2, 24, 50, device=DEV))
    with pytest.raises(ValueError, match="frames the encoder needs"):
        m.extract_embedding(xr.to(DEV), lengths=[x.shape[1], 1000, 2001])          # 1000 samples: 5 frames


@pytest.mark.parametrize("conv", ["f16x3", "f32"])
def test_encoder_train_gradients(conv):
    """One training step's gradients against fp64 autograd, both TRAIN_CONV modes: under f16x3 the first block reads the 24 band energies
    in a 32-channel tensor and hands the layer an input gradient -- a path no feature-fed encoder takes."""
    import ftdnn_ref
    from deeplip_amd import autograd_video as av
    av.TRAIN_CONV = conv
    m = _encoder().to(DEV).train()
    assert m._train_pad() == (32 if conv == "f16x3" else 24)
    x = _waves(8, 20, seed=22)
    gen = torch.Generator().manual_seed(5)
    gv, ga = torch.randn(8, 16, generator=gen), torch.randn(8, 16, generator=gen)
    p = ftdnn_ref.to64(m.state_dict(), grad=True)
    wv, wa = ref.encoder(x.double(), None, p, CONTEXTS, True, True, SINC)
    torch.autograd.backward([wv, wa], [gv.double(), ga.double()])
    xv, xa = m.extract_embedding(x.to(DEV))
    torch.autograd.backward([xv, xa], [gv.to(DEV), ga.to(DEV)])
    torch.cuda.synchronize()
    ev, ea = rel_err(xv.detach().cpu().numpy(), wv.detach().numpy()), rel_err(xa.detach().cpu().numpy(), wa.detach().numpy())
    errs = {}
    for name, q in m.named_parameters():
        if q.grad is None:
            assert p[name].grad is None and name.startswith("bn2."), name
            continue
        if name.startswith("tdnn.") and name.endswith("context_layer.bias"):
            assert float(q.grad.abs().max()) < 1e-4 * float(p[name.replace("context_layer.bias", "bn.bias")].grad.abs().max()) + 1e-5, name
            continue
        errs[name] = rel_err(q.grad.cpu().numpy(), p[name].grad.numpy())
    print(f"\nencoder train {conv}: xv {ev:.2e}, x_a {ea:.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert {"sinc.low_hz_", "sinc.band_hz_", "tdnn.0.context_layer.weight"} <= set(errs)
    assert ev < BAR_OUT and ea < BAR_OUT
    assert all(v < BAR_GRAD for v in errs.values()), errs


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
OV = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 48,
      "data.n_spk": 6, "data.utt_per_spk": 3, "data.train_from_waves": True, "data.test_ragged": True, "data.test_audio_frames": [20, 48],
      "train.bs": 8, "train.epoch": 1, "train.steps_per_epoch": 3, "train.crop_frames": None,
      "model.arch": "sincnet", "model.sincnet.hidden_dim": [32, 32, 32, 32, 64], "model.sincnet.embedding_dim": 16,
      "model.sincnet.sinc": {"kernel_size": 31}}
AUGMENT = {"snr_levels": [0, 10, 9999], "p_reverb": 0.5, "keep_power": True, "normalize": False, "max_taps": 8192}
SPEEDS = {"speeds": [0.9, 1.0, 1.1]}


class _EagerSteps:
    """Stands where the trainer keeps its recorded steps and issues every launch of every step from Python: the same trainer, the same
    optimizer kernel, the same batches -- only the replay is left out."""
    mode = "eager"

    def __init__(self, one_step):
        self.one_step = one_step

    def step(self, x, lab, key=None):
        return self.one_step(x, lab)

    def finish(self):
        pass


def _train_three(tmp_path, monkeypatch, recorded):
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = train_audio.Trainer(overrides={**OV, "train.graph_step": True}, arith_mode="f32")
    if not recorded:
        tr._steps = _EagerSteps(tr._one_step)
    low0 = tr.model.sinc.low_hz_.detach().cpu().clone()
    tr.current_epoch = 1
    tr._adjust_margin()
    loss = tr._train_epoch()
    torch.cuda.synchronize()
    params = {k: v.detach().cpu().clone() for k, v in list(tr.model.state_dict().items()) + [("crit." + k, v) for k, v in tr.criterion.state_dict().items()]}
    out = {"loss": loss, "mode": tr.last_epoch_stats["step_mode"], "params": params, "low0": low0,
           "in_optimizer": any(q is tr.model.sinc.low_hz_ for grp in tr.optim.param_groups for q in grp["params"])}
    tr.close()
    del tr
    gc.collect()
    return out


def test_recorded_step_equals_the_eager_step_bit_for_bit(tmp_path, monkeypatch):
    """Three steps, recorded (the first eager, two replays) and eager: the same bits in every parameter; the layer is inside the step and
    its parameters move."""
    g = _train_three(tmp_path, monkeypatch, True)
    e = _train_three(tmp_path, monkeypatch, False)
    assert g["mode"] == "graph" and e["mode"] == "eager"
    assert g["in_optimizer"] and e["in_optimizer"]
    diff = [k for k, v in e["params"].items() if not torch.equal(v, g["params"][k])]
    print(f"\nrecorded vs eager, three steps: loss {g['loss']!r} vs {e['loss']!r}; tensors that differ: {diff}")
    assert not diff and g["loss"] == e["loss"]
    assert not torch.equal(g["params"]["sinc.low_hz_"], g["low0"]) and bool(torch.isfinite(g["params"]["sinc.low_hz_"]).all())


FUSION_SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
                "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 60, "data.test_audio_frames": [20, 60],
                "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False,
                "model.audio_config.arch": "sincnet",
                "model.audio_config.sincnet": {"input_dim": 24, "hidden_dim": [32, 32, 64], "context": [[-2, -1, 0, 1, 2], [-2, 0, 2], [0]],
                                               "tdnn_layers": 3, "fc_layers": 3, "embedding_dim": 512, "pooling": "statistic", "bn_first": True,
                                               "sinc": {"kernel_size": 31}}}


def test_av_test_from_waveforms_with_the_sincnet_encoder(tmp_path, monkeypatch):
    """train_fusion's av_test with arch: sincnet: refused without test_from_waves; with it the speech rows are the encoder on each
    utterance's own waveform (checked one at a time), through RaggedExtractor(waves=True) on the layer's frame geometry."""
    import copy
    import train_fusion
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="test_from_waves"):
        train_fusion.Trainer("av_test", overrides=copy.deepcopy(FUSION_SMALL))
    tr = train_fusion.Trainer("av_test", overrides=dict(copy.deepcopy(FUSION_SMALL), **{"data.python_data_config.test_from_waves": True}))
    try:
        assert tr.model_audio.sinc is not None and tr.model_audio.sinc.kernel_size == 31
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        st = tr.extract_stats
        assert st["plans_recorded"] <= st["audio_shapes"] + st["video_shapes"]
        eer, _ = tr.eer_cos(ds, tr.lomgrid_tables, "cos")
        assert np.isfinite(eer) and 0.0 <= eer <= 1.0
        xa = tr.lomgrid_tables[1].emb
        assert bool(torch.isfinite(tr.lomgrid_tables[0].emb).all())
        for i in range(len(ds)):
            want = tr.model_audio.extract_embedding(torch.from_numpy(ds.wave_item(i)[None]).to(tr.device))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        tr.close()


def test_trainer_with_augmentation_and_speed_perturbation_to_an_eer(tmp_path, monkeypatch):
    """train_audio.Trainer with arch: sincnet from augmented, speed-perturbed waveforms: two steps, then the ragged test list through
    RaggedExtractor(waves=True) on the layer's frame geometry, to an EER."""
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    tr = train_audio.Trainer(overrides={**OV, "train.steps_per_epoch": 2, "data.augment": dict(AUGMENT), "data.speed_perturb": dict(SPEEDS)})
    try:
        assert tr._wave_fe is tr.model.sinc and tr._augment is not None and tr._speed is not None
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        st = tr.last_epoch_stats
        assert np.isfinite(loss) and st["from_waves"] is True and st["steps"] == 2 and st["speed_perturb"] == {"speeds": (0.9, 1.0, 1.1)}
        table = tr.extract_test_xv()
        assert tuple(table.emb.shape) == (12, 16) and bool(torch.isfinite(table.emb).all())
        assert tr.extract_stats and tr._extractor._held[1].frame_len == 400
        eer, _ = tr.eer()
        print(f"\nsincnet trainer: loss {loss:.4f}, EER {100 * eer:.2f}%")
        assert 0.0 <= eer <= 1.0
    finally:
        tr.close()
        del tr
        gc.collect()
