#!/usr/bin/env python3
"""train_video.py -- lip-clip encoder entry point (ResNet-18 + MS-TCN) on the MI355X engine.

Re-creation of the reference's train_video.py surface: the same argparse flags (:31-68), JSON model
config (conf/video_config.json), ``get_model`` (:173-190), ``extract_feats`` (:99-106), ``train``
(:108-169: Adam 3e-4 / wd 1e-4, CosineAnnealingLR(T_max=5) stepped PER ITERATION, CrossEntropy,
per-epoch ``<save_path>/<epoch+1>.pt`` state-dict checkpoints), ``main``.  Data are synthetic clips
produced with ``pad_packed_collate`` semantics (zero-pad to the longest clip + lengths list,
models/video_models/dataset.py:123-139); ``--rgb`` feeds uint8 [B,T,3,88,88] frames through the
GPU ingest kernel (gray + (x/255-0.421)/0.165).

What trains: the FULL model, as in the reference (``model.train()``: batch-statistics BatchNorm in stem /
trunk / TCN, learnable PReLU slopes, dropout; Adam over all parameters) -- every forward and backward
step a ``dlip_*`` launch (deeplip_amd/autograd_video.py: conv dgrad / wgrad on the implicit-GEMM kernels,
train-mode BN, PReLU, max-pool, pooling kernels), pinned by a golden step captured from the reference
class (tests/test_train_video_gpu.py).  ``--head-only`` trains the classifier layer ``tcn.tcn_output`` on
frozen eval-mode features instead (the fast path on the fused inference kernels).  Under
``torch.distributed.run`` every rank draws its own batches and the gradients are averaged by bucketed
all-reduce per step over RCCL (the reference uses DataParallel: train_video.py:196).
Round 6: the optimisation step is RECORDED once per batch shape and replayed as one HIP graph by default (``--eager-step`` keeps the
loop of eager launches; deeplip_amd/train_plan.py), the next batch's host-to-device copies run behind the step in flight, metrics stay
on the device between ``--display`` points; ``--arith auto|f16x3|f32`` (default: $DLIP_ARITH, the config's "arith", auto) picks the
engine's arithmetic (deeplip_amd/arith.py).  ``--device cpu`` runs the plumbing only (config -> model -> batches -> optimiser/scheduler ->
checkpoint round trip) because the engine has no CPU arithmetic by design.
``--time-masks`` / ``--cutouts`` / ``--mixup-alpha`` (with their widths, ``--mask-fill``; all off by default) augment the full-model training
batches on the device (deeplip_amd/clip_augment.py): time masks, cutout, and mixup with the mixed criterion.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from deeplip_amd import ops, train_loop as tl, weightgen as wg  # noqa: E402
from models.video_models.model import Lipreading  # noqa: E402

SEED = 1


def load_args(argv=None):
    p = argparse.ArgumentParser(description="Lipreading on the deeplip_amd engine")
    p.add_argument("--dataset", default="lomgrid", help="dataset selection")
    p.add_argument("--num-classes", type=int, default=54, help="Number of classes (database/lomgrid_54SpeakerLabel.txt)")
    p.add_argument("--label-path", type=str, default=None, help="Path to txt file with labels")
    p.add_argument("--backbone-type", type=str, default="resnet", choices=["resnet", "shufflenet"])
    p.add_argument("--relu-type", type=str, default="prelu", choices=["relu", "prelu"])
    p.add_argument("--width-mult", type=float, default=1.0)
    p.add_argument("--lr", type=float, default=0.0003)
    p.add_argument("--maxepoch", type=int, default=1)
    p.add_argument("--tcn-kernel-size", type=int, nargs="+")
    p.add_argument("--tcn-num-layers", type=int, default=4)
    p.add_argument("--tcn-dropout", type=float, default=0.2)
    p.add_argument("--tcn-dwpw", default=False, action="store_true")
    p.add_argument("--tcn-width-mult", type=int, default=1)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--model-path", type=str, default=None, help="Pretrained model pathname (bare state_dict)")
    p.add_argument("--extract-feats", default=False, action="store_true")
    p.add_argument("--mouth-patch-path", type=str, default=None)
    p.add_argument("--mouth-embedding-out-path", type=str, default=None)
    p.add_argument("--config-path", type=str, default=os.path.join(ROOT, "conf/video_config.json"))
    p.add_argument("--display", type=int, default=1)
    p.add_argument("--save-path", type=str, default="exp/video/epoch")
    # build-owned
    p.add_argument("--device", default="gpu", choices=["gpu", "cpu"])
    p.add_argument("--gpus", type=int, default=1, help="GPUs of this node, one process each over RCCL (the reference: "
                   "nn.DataParallel over every visible GPU, train_video.py:206-207); N > 1 starts its own N-rank job")
    p.add_argument("--steps", type=int, default=2, help="synthetic iterations per epoch")
    p.add_argument("--frames", type=int, default=29)
    p.add_argument("--rgb", action="store_true",
                   help="feed uint8 RGB frames [B,T,3,S,S] (S = --frame-size) through the ingest kernel: model.train() batches get the "
                        "reference's train pipeline -- RandomCrop(88) + HorizontalFlip(0.5) per clip, dataloaders.py:13-17 -- everything "
                        "else the val pipeline's CenterCrop(88)")
    p.add_argument("--frame-size", type=int, default=96, help="side of the synthetic uint8 mouth crops (LRW ROIs are 96 x 96)")
    p.add_argument("--head-only", action="store_true", help="train tcn.tcn_output on frozen eval-mode features")
    p.add_argument("--graph-step", action="store_true",
                   help="(the default since round 6; kept for old command lines) record the optimisation step and replay it as one HIP graph")
    p.add_argument("--eager-step", action="store_true",
                   help="issue every launch of every step from Python instead of replaying a recorded step (deeplip_amd.train_plan: one "
                        "recorded HIP graph per batch shape, recorded the second time a shape is met; the default for full-model training)")
    p.add_argument("--data-cache", type=int, default=0, metavar="N",
                   help="synthetic source: generate N batches once, keep them in pinned host memory and cycle through them (the numpy "
                        "generator makes ~30 clips/s; a run that measures the TRAINER rather than the generator uses this)")
    # training-time augmentation of the clips on the device (deeplip_amd/clip_augment.py): all off by default
    p.add_argument("--time-masks", type=int, default=0, help="time masks per clip (frames replaced by the fill value)")
    p.add_argument("--time-mask-width", type=int, default=0, help="the widest time mask, in frames")
    p.add_argument("--time-mask-ratio", type=float, default=1.0, help="a time mask is no wider than this share of its clip")
    p.add_argument("--cutouts", type=int, default=0, help="cutout rectangles per clip (the same rectangle in every frame)")
    p.add_argument("--cutout-size", type=int, default=0, help="the largest side of a cutout, in pixels of the 88 x 88 crop")
    p.add_argument("--mask-fill", type=str, default="mean", choices=["zero", "mean"], help="what a masked pixel holds: 0 or the clip's own mean")
    p.add_argument("--mixup-alpha", type=float, default=0.0, help="> 0: mixup of clip pairs, lam ~ Beta(alpha, alpha) per batch, mixed criterion")
    from deeplip_amd import arith
    arith.add_argument(p)
    args = p.parse_args(argv)
    args.clip_augment = clip_augment_options(args)
    return args


def clip_augment_options(args):
    """The keyword arguments of ``deeplip_amd.clip_augment.ClipAugment`` the augmentation flags name, or None with every one of them
    at its off value (the run is then today's, launch for launch).  A set of flags that would do nothing, a value out of range and
    ``--head-only`` beside them raise ValueError."""
    if not (args.time_masks or args.time_mask_width or args.cutouts or args.cutout_size or args.mixup_alpha):
        return None
    from deeplip_amd.clip_augment import ClipAugment
    kw = dict(time_masks=args.time_masks, time_width=args.time_mask_width, time_ratio=args.time_mask_ratio, cutouts=args.cutouts,
              cut_size=args.cutout_size, fill=args.mask_fill, mixup_alpha=args.mixup_alpha, crop=88)
    ClipAugment(**kw)           # validates
    if args.head_only:
        raise ValueError("train_video: the clip augmentation flags apply to full-model training batches; --head-only trains on frozen "
                         "eval-mode features")
    return kw


def load_json(path):
    with open(path) as f:
        return json.load(f)


def get_model(args):
    """train_video.py:173-190."""
    j = load_json(args.config_path)
    args.backbone_type, args.width_mult, args.relu_type = j["backbone_type"], j["width_mult"], j["relu_type"]
    tcn_options = {"num_layers": j["tcn_num_layers"], "kernel_size": j["tcn_kernel_size"], "dropout": j["tcn_dropout"],
                   "dwpw": j["tcn_dwpw"], "width_mult": j["tcn_width_mult"]}
    return Lipreading(num_classes=args.num_classes, tcn_options=tcn_options, backbone_type=args.backbone_type,
                      relu_type=args.relu_type, width_mult=args.width_mult, extract_feats=args.extract_feats)


def pad_packed_collate(batch):
    """dataset.py:123-139 semantics: sort by length (desc), zero-pad to the longest, lengths list."""
    batch = sorted(batch, key=lambda x: x[0].shape[0], reverse=True)
    lengths = [a.shape[0] for a, _ in batch]
    data = np.zeros((len(batch), lengths[0]) + batch[0][0].shape[1:], dtype=batch[0][0].dtype)
    for i, (a, _) in enumerate(batch):
        data[i, :a.shape[0]] = a
    return torch.from_numpy(data), lengths, torch.LongTensor([b for _, b in batch])


def synthetic_batch(args, it, rgb=False):
    r = np.random.Generator(np.random.PCG64([SEED, it]))
    items = []
    for i in range(args.batch_size):
        spk = int(r.integers(args.num_classes))
        T = args.frames if i == 0 else int(r.integers(max(2, args.frames // 3), args.frames + 1))
        size = args.frame_size if rgb else 88
        clip = wg.video_input(1, T, size, key=f"tv.{it}.{i}", speakers=[spk])[0, 0]          # [T,S,S] normalised gray
        if rgb:
            g = np.clip((clip * 0.165 + 0.421) * 255.0, 0, 255).astype(np.uint8)
            clip = np.repeat(g[:, None], 3, axis=1)                                            # [T,3,S,S] uint8: the loader's frames
        items.append((clip, spk))
    return pad_packed_collate(items)


def mixed_ce_loss(logits, labels_a, labels_b, lam):
    """Mixup's criterion: lam CE(logits, a) + (1 - lam) CE(logits, b), ``lam`` a float32 device tensor [1] read on the device (a
    recorded step follows new draws without being re-recorded)."""
    from deeplip_amd import autograd as ag
    return lam[0] * ag.margin_ce_loss(logits, labels_a, 1.0, 0.0) + (1.0 - lam[0]) * ag.margin_ce_loss(logits, labels_b, 1.0, 0.0)


def extract_feats(model, clip_thw, device):
    """:99-106: model(FloatTensor(data)[None,None], lengths=[T]) with extract_feats=True."""
    model.eval()
    x = torch.as_tensor(clip_thw, dtype=torch.float32)[None, None].to(device)
    y = model(x, lengths=[x.shape[2]])
    from deeplip_amd import _lib
    _lib.check_range(sync=True)           # the caller consumes y next: a range report of this very forward surfaces now
    return y


def build_step(model, args, device, full):
    """-> (Adam over what trains, one optimisation step ``step(x, *targets, lengths)``, its recorded form or None for the eager loop)."""
    from deeplip_amd import autograd as ag, dist as ddist, trainer_common as tc
    head = model.tcn.tcn_output
    if not full:
        for p in model.parameters():
            p.requires_grad = False
        for p in head.parameters():
            p.requires_grad = True
    params = [p for p in model.parameters() if p.requires_grad]
    # DP: gradients live in flat buckets whose all-reduces (RCCL) start while backward is still running
    buckets = ddist.GradBuckets(params) if (ddist.active() and device.type != "cpu") else None
    recorded = not bool(getattr(args, "eager_step", False)) and full and tl.records_with(buckets)
    optimizer = tc.make_optimizer("adam", params, {"init_lr": args.lr, "weight_decay": 1e-4}, recorded, device)      # (:112-113)

    def forward_loss(x, *targets):      # targets: labels -- mixup: labels_a, labels_b, lam (read on the device by every replay) -- then lengths
        *targets, lengths = targets
        if full:
            logits = model(x, lengths=lengths)                      # (:140) whole graph on the engine
        else:
            with torch.no_grad():
                pooled = model.classifier_features(x, lengths)      # frozen stem + trunk + MS-TCN
            logits = ag.linear(pooled, head.weight, head.bias)      # tcn_output (model.py:27)
        loss = mixed_ce_loss(logits, *targets) if len(targets) == 3 else ag.margin_ce_loss(logits, targets[0], 1.0, 0.0)      # (:115,143)
        return loss, logits

    step = tl.optim_step(forward_loss, optimizer, lambda: buckets)
    plan = tl.recorded_steps(step, [model], [optimizer], buckets, device, branch_streams=buckets is None) if recorded else None
    return optimizer, step, plan


class _Batches:
    """The synthetic loader behind train() (``--data-cache N``: its first N batches generated once, pinned, walked cyclically) and its
    batches' way to the step: ``stage(i)`` starts batch i's copies behind the running step, ``take`` forms the clip the model takes."""

    def __init__(self, args, world, rank, device, full):
        from deeplip_amd.clip_augment import ClipAugment
        self.args, self.world, self.rank, self.full, self.rgb = args, world, rank, full, args.rgb
        self.ring, self.prefetch, self.frontend = tl.BatchRing(self.make, getattr(args, "data_cache", 0)), tl.Prefetch(device), None
        self.pin = self.ring.n > 0 and device.type != "cpu"
        self.aug = ClipAugment(**args.clip_augment) if full and getattr(args, "clip_augment", None) else None
        self.crop_rng = random.Random(SEED + rank)     # the train pipeline's crop / flip draws (the reference: the `random` module, preprocess.py)
        self.aug_rng = np.random.default_rng(SEED + rank)

    def make(self, k):      # (inputs, lengths, labels) as pad_packed_collate hands them over (dataset.py:123-139)
        b = synthetic_batch(self.args, k * self.world + self.rank, self.rgb)        # (the module's global as it is now: a test swaps it)
        return (b[0].pin_memory(), b[1], b[2]) if self.pin else b

    def stage(self, i):
        inputs, lengths, labels = self.ring.get(i)
        host = {"raw": inputs, "lab": labels, "ln": torch.as_tensor(lengths, dtype=torch.int32), "lengths": lengths}
        if self.rgb and self.full:
            host["cp"] = torch.from_numpy(ops.draw_clip_params(inputs.shape[0], inputs.shape[-2], inputs.shape[-1], 88, rng=self.crop_rng))
        if self.aug is not None:            # its draws travel under their own names: draws, and perm and lam under mixup
            host.update((k, torch.from_numpy(v)) for k, v in self.aug.draw(inputs.shape[0], self.aug_rng).items())
        return self.prefetch.stage(host)

    def take(self, staged):
        """-> (x [B,1,T,88,88], the targets: (labels,) or mixup's (labels_a, labels_b, lam), lengths on the device, on the host)."""
        b = self.prefetch.take(staged)
        raw, ln, targets = b["raw"], b["ln"], (b["lab"],)
        if self.aug is not None:
            # time masks, cutout and mixup from the loader's frames (under --rgb with the crop and flip drawn in stage), one stage
            ap = {k: b[k] for k in ("draws", "perm", "lam") if k in b}
            x = self.aug(raw, clip_params=b["cp"], lengths=ln, params=ap) if self.rgb else self.aug(raw.unsqueeze(1), lengths=ln, params=ap)
            if self.aug.mixup:
                targets = self.aug.mix_targets(b["lab"], ap)
        elif self.rgb:
            # uint8 frames -> normalised 88 x 88 gray clips on the GPU: RandomCrop + HorizontalFlip per clip while the model
            # trains (dataloaders.py:13-17), CenterCrop otherwise (:19-24); padding frames = zeros of the normalised clip
            from deeplip_amd.frontend import VideoFrontend
            self.frontend = self.frontend or VideoFrontend(88)
            x = self.frontend(raw, clip_params=b.get("cp"), lengths=ln)
        else:
            x = raw.unsqueeze(1)                                                                    # :125
        return x, targets, ln, b["lengths"]


def run_epochs(model, args, device, rank, full, batches, optimizer, step, plan, sched):
    """The loop of train() -> ((last loss, logits shape) or None, (steps timed, their seconds) or None): metrics on the device between
    ``--display`` points, throughput counted from the 4th step on (a shape's first step is eager, its second records)."""
    import time
    gpu = device.type != "cpu"
    total_steps = int(args.maxepoch) * args.steps
    staged = batches.stage(0) if gpu and total_steps > 0 else None
    last_loss = last_shape = None
    mark_at, t_mark, t_end = min(3, max(total_steps - 1, 0)), None, None
    for epoch in range(int(args.maxepoch)):
        meter = tl.EpochMeter(device)
        model.train() if full else model.eval()                                                # (:129)
        for it in range(args.steps):
            gi = epoch * args.steps + it
            if not gpu:     # plumbing: the batch as the collate hands it over (the prefetch passes it through), no forward
                b = batches.prefetch.take(batches.stage(gi))
                print(f"[plumbing] batch {tuple(b['raw'].shape)} lengths {b['lengths']} labels {b['lab'].tolist()} lr {sched.get_last_lr()}")
                optimizer.step(); sched.step()
                continue
            if gi == mark_at:
                torch.cuda.synchronize(device)
                t_mark = time.perf_counter()
            x, targets, ln, lengths = batches.take(staged)
            if plan is not None:
                loss, logits = plan.step(x.contiguous(), *targets, ln)
            else:
                loss, logits = step(x, *targets, lengths)
            sched.step()                                                        # per-iteration (:147)
            _, pred = torch.max(torch.softmax(logits.detach(), 1), 1)           # (:145)
            hits = (pred == targets[0]).sum()
            if len(targets) == 3:       # the mixed criterion's accuracy: lam (pred == a) + (1 - lam) (pred == b)
                lam = targets[2][0].double()
                hits = lam * hits + (1.0 - lam) * (pred == targets[1]).sum()
            meter.add(loss, hits, targets[0].shape[0])
            last_loss, last_shape = loss.detach().clone(), tuple(logits.shape)
            staged = batches.stage(gi + 1) if gi + 1 < total_steps else None    # the next batch's copies run behind this step
            if it % args.display == 0 or it + 1 == args.steps:
                if plan is not None:
                    plan.finish()                                               # waits; a range report of the f16x3 arithmetic surfaces here
                a0, a1, a2 = meter.read()
                if rank == 0 and it % args.display == 0:
                    print(f"epoch {epoch} it {it} loss {a0 / a2:.4f} acc {a1 / a2:.3f} lr {float(sched.get_last_lr()[0]):.2e}"
                          f"{' (replayed)' if plan is not None and plan.last.recorded else ''}", flush=True)
        if gpu and epoch + 1 == int(args.maxepoch):
            torch.cuda.synchronize(device)
            t_end = time.perf_counter()                                                        # (the checkpoint below is not a step)
        if rank == 0:
            os.makedirs(args.save_path, exist_ok=True)
            torch.save(model.state_dict(), os.path.join(args.save_path, f"{epoch + 1}.pt"))  # (:169)
    last = (float(last_loss), last_shape) if last_loss is not None else None
    timed = (total_steps - mark_at, t_end - t_mark) if t_mark is not None and t_end is not None and total_steps > mark_at else None
    return last, timed


def train(model, args, device):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    full = not args.head_only and device.type != "cpu"
    batches = _Batches(args, world, rank, device, full)
    optimizer, step, plan = build_step(model, args, device, full)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=5, eta_min=4e-08)      # (:114)
    train.last_stats, train.last_plan = None, plan
    if device.type == "cpu" and rank == 0:
        print("[plumbing] --device cpu exercises config / collate / optimizer / scheduler / checkpoint plumbing ONLY (BASELINE config C1): the "
              "engine has no CPU arithmetic path by design, so no forward runs and no loss or logits exist here; the same command on "
              "--device gpu computes them (C1-size run: tests/test_entrypoints.py::test_train_video_gpu_two_steps[c1-size]).")
    last, timed = run_epochs(model, args, device, rank, full, batches, optimizer, step, plan, sched)
    if timed is not None:
        steps, dt = timed
        train.last_stats = {"clips_per_s": steps * args.batch_size * world / dt, "ms_per_step": 1e3 * dt / steps, "steps_timed": steps,
                            "step_mode": plan.mode if plan is not None else "eager", "global_batch": args.batch_size * world}
        if rank == 0:
            print("train: {:.1f} clips/s, {:.2f} ms/step over the last {} steps [{}]".format(
                train.last_stats["clips_per_s"], train.last_stats["ms_per_step"], steps, train.last_stats["step_mode"]), flush=True)
    if rank == 0 and device.type != "cpu":
        how = ("recorded steps: " + str(plan.summary())) if plan is not None else "eager steps"
        print(f"train: {how}", flush=True)
    return last


def main(argv=None):
    args = load_args(argv)
    from deeplip_amd import arith
    mode = arith.configure(args.arith, load_json(args.config_path).get("arith"))     # before the first weight pack
    if args.device == "gpu" and args.gpus > 1:
        from deeplip_amd import launch
        rc = launch.maybe_self_launch(os.path.abspath(__file__), list(sys.argv[1:] if argv is None else argv), args.gpus)
        if rc is not None:      # this process was the launcher of the N-rank job; nothing here touched the GPU
            sys.exit(rc)
    # the reference seeds once (train_video.py:70-73); under DP every rank needs its own dropout masks
    torch.manual_seed(SEED + int(os.environ.get("RANK", "0"))); np.random.seed(SEED)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))) if args.device == "gpu" else torch.device("cpu")
    if args.device == "gpu" and not torch.cuda.is_available():
        raise RuntimeError("no ROCm GPU visible: use --device cpu for the plumbing-only run")
    model = get_model(args)
    if args.model_path and os.path.exists(args.model_path):
        model.load_state_dict(torch.load(args.model_path, map_location="cpu"))
    else:
        sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, prefix="video.")
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.to(device)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    in_job = "RANK" in os.environ            # any torch.distributed.run job joins its process group, a one-rank one included
    if in_job and args.device == "gpu":
        import torch.distributed as dist
        from deeplip_amd import dist as ddist
        torch.cuda.set_device(device)
        ddist.init_from_env(device)
        ddist.broadcast_params(list(model.parameters()) + list(model.buffers()))
    if args.extract_feats and args.mouth_patch_path:
        out = extract_feats(model, np.load(args.mouth_patch_path)["data"], device)
        if args.mouth_embedding_out_path:
            np.savez(args.mouth_embedding_out_path, data=out.cpu().numpy())
        return out
    res = train(model, args, device)
    if in_job and args.device == "gpu":
        import torch.distributed as dist
        dist.barrier()
    # checkpoint round trip (bare state_dict, as the reference saves it)
    ck = os.path.join(args.save_path, f"{int(args.maxepoch)}.pt")
    model.load_state_dict(torch.load(ck, map_location="cpu"))
    if int(os.environ.get("RANK", "0")) == 0:
        print("done:", res, "checkpoint", ck)
    if in_job and args.device == "gpu":
        import torch.distributed as dist
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
