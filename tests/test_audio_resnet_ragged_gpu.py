"""Ragged batches through the ResNet speech encoder (`arch: resnet`; -m gpu).

The reference's test loop feeds one utterance at a time at its own length (train_audio.py:343-373).  The engine takes the zero-padded
batch + length vector instead and must return, row by row, what that loop returns: every layer's input is kept zero behind each
utterance's end (dlip_time_tail_zero_f32 after every convolution; after k stride-2 stages the length is ((L - 1) >> k) + 1) and the
pooling divides by each utterance's own frame count (dlip_avgpool_time_ragged_f32).

Bars: the two kernels against plain torch (bit-identical / 1e-6 element-wise, the bar test_ragged_gpu.py holds time_mean with lengths to);
model rows against the engine run on the utterance alone, rel_err < 1e-6 (the ragged-rows bar of test_ragged_gpu.py), and against the
oracle on the utterance alone, rel_err < 1e-4 (the bar of test_audio_resnet_gpu.py); a replayed plan bit-identical to the eager call.
"""
import numpy as np
import pytest
import torch

from conftest import assert_close_rel, rel_err
from deeplip_amd import weightgen as wg
from oracle import deeplip_oracle as O
from test_audio_resnet_gpu import _net

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(3, 3, 7, 4), (2, 5, 16, 32), (4, 2, 9, 64), (1, 1, 1, 256)]      # [N,H,W,C]; the second one in the split format


def _length_vectors(N, W, shift):
    """Input lengths that between them hold: W << shift (nothing to zero), 1, one short of a power of two, one above the maximum
    (clamped) -- as many vectors of N entries as it takes to use all four."""
    top = W << shift
    pow2 = 1 << (top.bit_length() - 1)                # the largest power of two <= top
    cands = [top, 1, max(pow2 - 1, 1), top + 3]
    return [[cands[(s + i) % 4] for i in range(N)] for s in range(0, 4, N)]


def _valid(L, shift, W):
    return ((min(max(L, 1), W << shift) - 1) >> shift) + 1


@pytest.fixture(params=["f32", "f16x3"])
def mode(request):
    from deeplip_amd import packing
    packing.set_precision(request.param)
    yield request.param
    packing.set_precision("f32")


# ------------------------------------------------------------------------------------------ the kernels themselves
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_time_tail_zero_vs_torch_masking_bit_identical(shape, shift):
    """NaN where the kernel must write, random bits elsewhere: untouched positions keep their bits, tails are exactly +0."""
    from deeplip_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(17 + shift)
    base = torch.randn(shape, generator=g).to(DEV)
    if shape == SHAPES[1]:
        base = ops.split_pack(base)                   # (hi, lo) fp16 pairs in the fp32 container: its zero is all-zero bits too
    for lens in _length_vectors(N, W, shift):
        x, want = base.clone(), base.clone()
        for n, L in enumerate(lens):
            Lk = _valid(L, shift, W)
            x[n, :, Lk:, :] = float("nan")
            want[n, :, Lk:, :] = 0.0
        got = ops.time_tail_zero(x, torch.tensor(lens, dtype=torch.int32, device=DEV), shift)
        torch.cuda.synchronize()
        assert got is x
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (shape, shift, lens)


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_time_ragged_vs_fp64_torch_mean(shape, shift):
    from deeplip_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(29 + shift)
    x = torch.randn(shape, generator=g)
    xd = x.to(DEV)
    for lens in _length_vectors(N, W, shift):
        got = ops.avgpool_time_ragged(xd, torch.tensor(lens, dtype=torch.int32, device=DEV), shift).cpu()
        assert got.shape == (N, C)
        for n, L in enumerate(lens):
            Lk = _valid(L, shift, W)
            want = x[n, :, :Lk].double().mean(dim=(0, 1)).float()
            assert_close_rel(got[n].numpy(), want.numpy(), rtol=1e-6, what=f"ragged pool {shape} shift {shift} len {L}")


# ------------------------------------------------------------------------------------------ the encoder
def _ragged_batch(lengths, F, T, key):
    """[B,1,F,T]: utterance b = its own seeded [F,L_b] features, non-zero junk behind it."""
    x = 37.0 * wg.audio_input(len(lengths), F, T, key=key + ".junk") + 1.0
    items = []
    for b, L in enumerate(lengths):
        it = wg.audio_input(1, F, L, key=f"{key}.{b}", speakers=[b % 5])[0]
        x[b, :, :L] = it
        items.append(torch.from_numpy(it[None, None]))                      # [1,1,F,L_b]
    return torch.from_numpy(x).unsqueeze(1), items


def _check_rows(net, sd, lengths, key):
    from deeplip_amd import _lib
    x, items = _ragged_batch(lengths, 24, 37, key)
    assert all(bool((x[b, :, :, L:] != 0).all()) for b, L in enumerate(lengths))       # the padding really is junk
    e, e2 = net.extract_embedding(x.to(DEV), lengths=lengths)
    e_dev, _ = net.extract_embedding(x.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    _lib.check_range(sync=True)
    assert e.shape == (len(lengths), 256) and e is e2 and bool(torch.isfinite(e).all())
    assert torch.equal(e, e_dev)                                           # host list and device vector: the same launches
    for b, it in enumerate(items):
        one = net.extract_embedding(it.to(DEV))[0]
        _lib.check_range(sync=True)
        with torch.no_grad():
            ref = O.audio_resnet_embedding(sd, it)
        a, o = rel_err(e[b:b + 1].cpu().numpy(), one.cpu().numpy()), rel_err(e[b:b + 1].cpu().numpy(), ref.numpy())
        print(f"\nrow {b} (L={lengths[b]}): vs alone {a:.3e}, vs oracle {o:.3e}")
        assert a < 1e-6, f"row {b} (L={lengths[b]}) vs the utterance alone: {a:.3e}"
        assert o < 1e-4, f"row {b} (L={lengths[b]}) vs the oracle on the utterance alone: {o:.3e}"
    # other junk in the padding, the same bits
    x2 = x.clone()
    for b, L in enumerate(lengths):
        x2[b, :, :, L:] = -3.0 * x2[b, :, :, L:] + 2.0
    e3 = net.extract_embedding(x2.to(DEV), lengths=lengths)[0]
    torch.cuda.synchronize()
    assert torch.equal(e3, e)


def test_ragged_rows_equal_the_reference_loop_f32():
    """Shipped config, F = 24, padded T = 37, lengths down to 1 and 2 frames (2 -> 1 -> 1 through the stride-2 stages; 19 -> 10 -> 5:
    odd and even ends), exact-fp32 arithmetic."""
    from deeplip_amd import packing
    packing.set_precision("f32")
    net, sd = _net()
    net.eval()
    _check_rows(net, sd, [37, 36, 19, 2, 1], "aresnet.ragged")


def test_ragged_rows_equal_the_reference_loop_f16x3():
    """The same in the split-fp16 arithmetic, with lengths whose one-at-a-time runs stay inside the split format's range at
    wg.audio_input's gain."""
    from deeplip_amd import packing
    packing.set_precision("f16x3")
    try:
        net, sd = _net()
        net.eval()
        _check_rows(net, sd, [37, 36, 23, 16, 9], "aresnet.ragged")
    finally:
        packing.set_precision("f32")


def test_one_recorded_plan_replays_with_new_lengths(mode):
    """Nothing on the path reads the lengths on the host: a plan recorded at one (B, T) with a device length vector replays with a
    second one, bit-identical to the eager call on the new lengths."""
    from deeplip_amd.plan import StepPlan
    net, _ = _net()
    net.eval()
    la, lb = [37, 30, 23, 16], [19, 37, 9, 28]
    xa, _ = _ragged_batch(la, 24, 37, "aresnet.plan.a")
    xb, _ = _ragged_batch(lb, 24, 37, "aresnet.plan.b")
    ins = (xa.to(DEV), torch.tensor(la, dtype=torch.int32, device=DEV))
    ins2 = (xb.to(DEV), torch.tensor(lb, dtype=torch.int32, device=DEV))

    def step(a, l):
        return net.extract_embedding(a, lengths=l)[0]

    plan = StepPlan(step, *ins)
    try:
        first = plan.run().clone()
        torch.cuda.synchronize()
        assert torch.equal(first, step(*ins))
        got = plan(*ins2).clone()
        torch.cuda.synchronize()
        want = step(*ins2)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and not torch.equal(got, first)
    finally:
        plan.close()


def test_lengths_are_validated():
    from deeplip_amd import ops
    net, _ = _net()
    net.eval()
    x = torch.zeros(2, 1, 24, 37, device=DEV)
    with pytest.raises(ValueError):
        net.extract_embedding(x, lengths=[37])                 # one length per utterance
    with pytest.raises(ValueError):
        net.extract_embedding(x, lengths=[37, 0])              # the shortest utterance is one frame
    with pytest.raises(ValueError):
        net.extract_embedding(x, lengths=[38, 5])              # longer than the padded batch
    with pytest.raises(TypeError):
        net.extract_embedding(x, lengths=torch.tensor([37, 5], device=DEV))     # a device vector must be int32
    lens = torch.tensor([37, 5], dtype=torch.int32, device=DEV)
    blk = net._blocks()[0]
    with pytest.raises(ValueError):
        blk.run(torch.zeros(2, 24, 37, 64, device=DEV), {}, pool_group=8, time_lengths=(lens, 0))
    with pytest.raises(ValueError):
        ops.time_tail_zero(torch.zeros(2, 3, 5, 6, device=DEV), lens, 0)        # C % 4
    net.train()
    with pytest.raises(NotImplementedError):
        net.extract_embedding(x, lengths=[37, 5])


# ------------------------------------------------------------------------------------------ the trainer
def test_train_audio_resnet_extracts_its_ragged_test_list(tmp_path, monkeypatch, arith_mode):
    """`arch: resnet` with data.test_ragged at its shipped value: the test list goes through the RaggedExtractor and every row of the
    table equals the model run on that utterance alone (2e-6: the bar test_ragged_gpu.py uses behind a further layer + L2 norm)."""
    import train_audio
    from deeplip_amd import ops
    monkeypatch.chdir(tmp_path)
    tr = train_audio.Trainer(overrides={"model.arch": "resnet", "data.feat_dim": 24, "data.test_speakers": 3, "data.test_utt_per_spk": 2,
                                        "data.trials": 30, "data.trial_targets": 6, "data.audio_frames": 60, "data.n_spk": 5,
                                        "data.utt_per_spk": 2, "data.test_audio_frames": [40, 90], "train.bs": 4, "train.epoch": 1})
    try:
        ds = tr.voxtestset
        assert ds.ragged and len(set(int(l) for l in ds.audio_len)) > 1
        table = tr.extract_test_xv(batch=4)
        assert table.emb.shape == (6, 256) and bool(torch.isfinite(table.emb).all())
        st = tr.extract_stats
        assert st["audio_batches"] >= 1 and st["plans_recorded"] >= 1 and st["valid_audio_frames"] == int(ds.audio_len.sum())
        ce = tr.train_opts["loss"] == "CrossEntropy"
        tr.model.eval()
        with torch.no_grad():
            for i in range(len(ds)):
                xv, x_a = tr.model.extract_embedding(torch.from_numpy(ds.audio_item(i)[None]).to(DEV))
                want = x_a if ce else ops.l2_normalize(xv)
                torch.cuda.synchronize()
                e = rel_err(table.emb[i:i + 1].cpu().numpy(), want.cpu().numpy())
                assert e < 2e-6, f"utterance {i} (T={int(ds.audio_len[i])}): {e:.3e}"
    finally:
        tr.close()
