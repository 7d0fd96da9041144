"""Command line entry point: the reference's flags (BAR/main.py:83-97,
DAR/main.py:87-103, BR/main.py:77-92, BDR/main.py:77-93) plus the MI355X-native
extensions (SURVEY §5 config row, §7.4 decisions).

Launch (one process per GPU, RCCL over xGMI):
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py [flags]
CPU / gloo plumbing runs the same way with --device cpu.

Reference flags kept verbatim: --local-rank, --backend {nccl,gloo,mpi}, --epochs_local,
--epochs_global, --batch_size, --lr, --time_limit, --prev_fraction, --next_fraction,
--aggregation_type {equal,weighted}, --aggregation_by {gradients,weights},
--local_weight, --fixed_ratio, --gpu_weight (accepted, unused as in the reference),
--dist-url (accepted, unused).
"""
from __future__ import annotations

import argparse
import json
import math
import os

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ldnn: MI355X-native distributed DNN training")
    # ---- reference flags
    p.add_argument("--local-rank", "--local_rank", type=int, dest="local_rank", default=None)
    p.add_argument("--backend", type=str, default="auto", choices=["auto", "nccl", "gloo", "mpi"],
                   help="process-group backend; nccl = RCCL on ROCm; mpi maps to the default backend")
    p.add_argument("--epochs_local", type=int, default=5)
    p.add_argument("--epochs_global", type=int, default=20)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--time_limit", type=float, default=60.0)
    p.add_argument("--prev_fraction", type=float, default=0.5)
    p.add_argument("--next_fraction", type=float, default=0.5)
    p.add_argument("--aggregation_type", type=str, default="equal", choices=["equal", "weighted"])
    p.add_argument("--aggregation_by", type=str, default="gradients", choices=["gradients", "weights"])
    p.add_argument("--local_weight", type=float, default=0.5)
    p.add_argument("--fixed_ratio", type=float, default=None,
                   help="class-skewed ('disbalanced') partition with this fraction of fixed classes")
    p.add_argument("--gpu_weight", type=float, default=10, help="accepted for compatibility (unused)")
    p.add_argument("--dist-url", type=str, default=None, help="accepted for compatibility (unused)")
    # ---- extensions
    p.add_argument("--topology", type=str, default="allreduce", choices=["allreduce", "ring", "double_ring"])
    p.add_argument("--partition", type=str, default=None, choices=["balanced", "skewed"],
                   help="skewed requires --fixed_ratio (default 0.5)")
    p.add_argument("--partition_rule", type=str, default="reference_duration",
                   choices=["reference_duration", "throughput", "equal"])
    p.add_argument("--sync_every", type=str, default="global_epoch", choices=["global_epoch", "step"],
                   help="global_epoch = reference schedule (SURVEY Q1); step = per-step data parallelism")
    p.add_argument("--model", type=str, default="enhanced_cnn")
    p.add_argument("--dataset", type=str, default=None, help="cifar10 | mnist | imagenet | imagenet64 (synthetic "
                   "unless the CIFAR-10 binary files exist under --data_root)")
    p.add_argument("--n_train", type=int, default=None)
    p.add_argument("--n_test", type=int, default=None)
    p.add_argument("--data_root", type=str, default="data")
    p.add_argument("--optimizer", type=str, default="adam", choices=["adam", "adamw", "sgd", "lars", "lamb", "lion"],
                   help="lars: SGD-momentum with layer-wise adaptive rate scaling (per-tensor trust ratios); "
                        "lamb: Adam's direction with per-tensor trust ratios |w| / |u| (metrics.jsonl then logs "
                        "lamb_ratio_min / _median / _max per global epoch); lion: the sign of an interpolated "
                        "momentum with one moment buffer, betas (0.9, 0.99) and decoupled --weight_decay (use a "
                        "3-10x smaller --lr and a 3-10x larger --weight_decay than for adamw)")
    p.add_argument("--lamb_adapt_1d", action="store_true",
                   help="--optimizer lamb: also adapt tensors with dim() < 2 (biases, BatchNorm affine)")
    p.add_argument("--lars_trust", type=float, default=0.001,
                   help="--optimizer lars: trust coefficient of the ratio trust * |w| / (|g| + wd * |w| + eps).  "
                        "metrics.jsonl then logs lars_ratio_min / _median / _max per global epoch")
    p.add_argument("--lars_eps", type=float, default=1e-8)
    p.add_argument("--lars_adapt_1d", action="store_true",
                   help="--optimizer lars: also adapt tensors with dim() < 2 (biases, BatchNorm affine)")
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--clip_grad_norm", type=float, default=0.0,
                   help="clip the gradient by its global L2 norm (torch clip_grad_norm_ semantics) inside the fused "
                        "optimizer, and skip a step whose norm is not finite; 0 (default) = off.  metrics.jsonl then "
                        "logs grad_norm_last / grad_clipped_steps / grad_skipped_steps per global epoch")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing of the cross-entropy (torch semantics: targets eps / C + (1 - eps) * onehot, "
                        "0 <= eps <= 1) inside the fused loss kernel; 0 (default) = off.  The same criterion serves "
                        "validation and the final test, so the reported val / test losses are the smoothed ones "
                        "(accuracy is unaffected)")
    p.add_argument("--class_weights", type=str, default="none", metavar="{none,balanced,sqrt,W0,W1,...}",
                   help="class weights of the cross-entropy (torch's weight=) inside the fused loss kernel, against "
                        "class-skewed shards; none (default) = off, nothing is built.  balanced: n / (C_present * n_c) "
                        "over THIS rank's current training shard (absent classes get 0), recomputed at every global "
                        "epoch and after every re-partition, so ranks differ on purpose under --partition skewed; "
                        "sqrt: 1 / sqrt(n_c), scaled to a mean per-sample weight of 1; or one finite weight >= 0 per "
                        "class, comma-separated, written once.  The same criterion serves validation and the final "
                        "test, so the reported val / test losses are the weighted ones (accuracy is unaffected).  "
                        "metrics.jsonl then logs class_weight_min / class_weight_max per global epoch")
    p.add_argument("--focal_gamma", type=float, default=0.0, metavar="G",
                   help="focal loss (Lin et al. 2017) inside the fused loss kernel, against easy samples dominating "
                        "the gradient on class-skewed shards: a sample's loss is w[y] (1 - p)^G (-log p), p its "
                        "softmax probability of the true class, over the weight sum of the batch; G finite and >= 0, "
                        "0 (default) = off, the criterion is the one without it.  w comes from --class_weights (1 "
                        "without), whose per-epoch recomputation keeps working.  Not defined with --label_smoothing, "
                        "--mixup or --cutmix: those combinations exit.  The same criterion serves validation and the "
                        "final test, so the reported val / test losses are the focal ones (accuracy is unaffected)")
    p.add_argument("--dropout", type=float, default=0.0, metavar="P",
                   help="dropout at rate P (0 <= P < 1; 0 (default) = off, no module is built) after every hidden "
                        "layer of the MLPs, after LeNet-5's fc1 and fc2, in front of the classifier of the ResNets and "
                        "EnhancedCNNs, in one native pass each way (dropout.hip) whose mask is a counter hash of "
                        "(--seed, rank, global epoch, module, step): nothing is stored for the backward, a resumed run "
                        "replays the masks, and validation and the final test run without it")
    p.add_argument("--norm", choices=["batch", "group", "layer"], default="batch",
                   help="normalisation layer of the EnhancedCNNs and ResNets: batch (default, BatchNorm2d) or group "
                        "(GroupNorm under the same parameter names: statistics per sample, so the result does not "
                        "depend on which samples share a batch; no running statistics, train and eval are the same "
                        "function; native NHWC bf16 passes with the residual add and the ReLU fused, group_norm.hip).  "
                        "The MLPs and LeNet-5 have no normalisation layer and refuse group.  layer: the MLPs only -- a "
                        "LayerNorm over the width after every hidden Linear, with the activation fused (statistics per "
                        "row, native bf16 row passes, layer_norm.hip); every other model refuses it")
    p.add_argument("--gn_groups", type=int, default=32, metavar="G",
                   help="--norm group: number of channel groups (default 32); must divide every normalised width")
    p.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA",
                   help="Mixup of every training batch with a permutation of itself, lam ~ Beta(ALPHA, ALPHA), one "
                        "draw per batch, in one native pass (mix.hip) that also writes the class-probability targets "
                        "of the soft-target loss kernel; 0 (default) = off.  Training accuracy is then agreement with "
                        "the dominant label; validation and test use hard labels.  metrics.jsonl then logs "
                        "mix_lam_mean per global epoch")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA",
                   help="CutMix likewise: a box of area ~ 1 - lam comes from the permuted image; 0 (default) = off")
    p.add_argument("--mix_prob", type=float, default=1.0,
                   help="--mixup / --cutmix: probability that a batch is mixed at all")
    p.add_argument("--mix_switch_prob", type=float, default=0.5,
                   help="--mixup and --cutmix both on: probability that a mixed batch takes CutMix")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="keep an exponential moving average of the weights (decay d, 0 <= d < 1; 0 = off) on the "
                        "device, updated once per non-skipped optimizer step, and run every validation and the final "
                        "test on the averaged weights (BatchNorm running statistics are not averaged: the live ones "
                        "serve).  Each replica averages its own master; an end-of-epoch aggregation is one more jump "
                        "of the weights it follows.  metrics.jsonl then logs ema_updates / ema_a_last per global epoch")
    p.add_argument("--ema_no_warmup", action="store_true",
                   help="--ema_decay: use d from the first step on instead of d_t = min(d, (1 + c) / (10 + c)) after "
                        "c updates")
    p.add_argument("--fedprox_mu", type=float, default=0.0, metavar="MU",
                   help="FedProx (Li et al. 2020) against client drift between two aggregations: every rank "
                        "minimises its loss + MU / 2 * |w - w_round|^2, w_round its weights at the start of the global "
                        "epoch (behind the aggregation).  MU * (w - w_round) joins the gradient inside the fused "
                        "optimizer update, where weight decay does (the clip norm of --clip_grad_norm does not see "
                        "it); 0 = off.  For --partition skewed with several --epochs_local; not with --optimizer "
                        "lars | lamb, autograd path only.  metrics.jsonl then logs prox_mu / prox_drift_norm "
                        "(|w - w_round| before the aggregation) per global epoch")
    p.add_argument("--lr_schedule", type=str, default="none", choices=["none", "constant", "linear", "poly", "cosine"],
                   help="per-step learning-rate schedule inside the fused optimizer: a linear warm-up over "
                        "--warmup_steps, then constant, polynomial (linear: power 1) or cosine decay to "
                        "--lr_min_ratio at --lr_total_steps.  It multiplies the rate StepLR leaves (--step_size / "
                        "--gamma keep running per local epoch), counts only steps that updated the weights, and "
                        "replays from the hipGraphs without a host write.  metrics.jsonl then logs lr_last / "
                        "lr_sched_steps per global epoch; none (default) = off")
    p.add_argument("--warmup_steps", type=int, default=0, help="--lr_schedule: linear warm-up steps")
    p.add_argument("--warmup_start", type=float, default=0.0,
                   help="--lr_schedule: the warm-up runs from this fraction of the rate (step u of W uses "
                        "start + (1 - start) * u / W)")
    p.add_argument("--lr_total_steps", type=int, default=None,
                   help="--lr_schedule: the horizon in optimizer steps (default: global epochs x local epochs x the "
                        "initial train loader's length, printed at start; with --sync_every step on several ranks the "
                        "ranks agree on the steps a local epoch runs -- the shortest loader's, plus the tail step "
                        "when a rank holds more -- so that every rank schedules alike)")
    p.add_argument("--lr_min_ratio", type=float, default=0.0,
                   help="--lr_schedule: the floor of the decay, as a fraction of the rate")
    p.add_argument("--lr_power", type=float, default=2.0, help="--lr_schedule poly: the power")
    p.add_argument("--step_size", type=int, default=25, help="StepLR step (local epochs), BAR/main.py:54")
    p.add_argument("--gamma", type=float, default=0.1)
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="auto", help="auto | cpu | cuda")
    p.add_argument("--legacy_gossip", action="store_true", help="reproduce the reference's lost GPU gossip update")
    p.add_argument("--average_buffers", action="store_true", help="also average BN buffers in weight averaging")
    p.add_argument("--replace", nargs="?", const="on", default="auto", choices=["auto", "on", "off"],
                   help="sample the per-global-epoch re-partition with replacement.  auto (default) follows the "
                        "reference variant: on for class-skewed shards (DAR/DR/DDR dataloader.py:123,129) and for "
                        "the balanced double ring (BDR/dataloader.py:94,100), off for BAR/BR")
    p.add_argument("--no_repartition", action="store_true")
    p.add_argument("--check_every", type=int, default=20, help="steps between straggler-cutoff rounds")
    p.add_argument("--bucket_mb", type=float, default=32.0)
    p.add_argument("--grad_comm_dtype", choices=["fp32", "bf16"], default="fp32",
                   help="dtype of the per-step gradient all-reduce (bf16 halves the xGMI bytes)")
    p.add_argument("--shard_optimizer", choices=["auto", "on", "off"], default="auto",
                   help="per-step all-reduce DP of autograd models: reduce-scatter each gradient bucket, run the "
                        "fused optimizer on this rank's 1/N shard, all-gather the bf16 weights (ZeRO-1 style, "
                        "parallel/ddp.py); auto = on for GPU runs with --aggregation_type equal")
    p.add_argument("--oneshot_bytes", type=int, default=None,
                   help="RCCL runs on one node: SUM all-reduces of at most this many bytes use the one-shot IPC "
                        "kernel that reads every peer's copy over its own xGMI link (parallel/ipc.py); opt-in, "
                        "default 0 = off (env LDNN_ONESHOT_BYTES); 4194304 covers LeNet-5's whole gradient")
    p.add_argument("--augment", nargs="?", const="autoaugment", default="none",
                   choices=["none", "autoaugment", "flipcrop", "autoaugment+flipcrop"],
                   help="training-set augmentation in the native input kernel (augment.hip); bare --augment = "
                        "AutoAugment(CIFAR10), the reference's train transform (BAR/dataloader.py:16)")
    p.add_argument("--augment_val", action="store_true",
                   help="also augment the validation shard: the reference's split of an augmented train set "
                        "(BAR/dataloader.py:29-35) does that")
    p.add_argument("--out_dir", type=str, default="runs/latest")
    p.add_argument("--plots", type=str, default="Graphs", help="output folder of the six plots ('' to skip)")
    p.add_argument("--checkpoint_every", type=int, default=0)
    p.add_argument("--resume", type=str, default=None, help="checkpoint path or 'latest'")
    p.add_argument("--timeout", type=float, default=600.0, help="collective timeout (s): failure detection")
    p.add_argument("--no_eval", action="store_true")
    p.add_argument("--log_weights_digest", action="store_true",
                   help="end every rank's metrics file with a final_weights record: the sha256 of that rank's "
                        "state_dict (replicas of a per-step all-reduce run must report the same one)")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--graphs", dest="graphs", action="store_true", default=True,
                   help="(default) on a GPU, replay each training step from hipGraphs; with --sync_every step the "
                        "backward is a chain of graphs cut at the gradient buckets, each bucket's RCCL all-reduce "
                        "issued between two links (train/graphed.py GraphedDPStep).  CPU runs are always eager")
    p.add_argument("--no_graphs", dest="graphs", action="store_false", help="eager steps (one launch per kernel)")
    p.add_argument("--engine", choices=["auto", "autograd", "static"], default="auto",
                   help="static: MLP models run on the graph-captured static engine (train/static_mlp.py: native "
                        "kernels, fused loss + optimizer, per-step DP = its own RCCL reduce-scatter / sharded update "
                        "/ all-gather); autograd: the generic module path; auto: static for MLPs on a GPU whenever "
                        "the topology / schedule allows it")
    p.add_argument("--ref_samples_per_s", type=float, default=None,
                   help="one GPU's measured samples/s for this model and batch: metrics.jsonl then also logs the "
                        "data-parallel scaling efficiency per global epoch")
    p.add_argument("--trace", action="store_true",
                   help="roctx ranges per phase + HIP-event phase timers (summary in metrics.jsonl)")
    return p


def resolve_replace(flag: str, fixed_ratio, topology: str) -> bool:
    """--replace auto -> the reference variant's sampling (see the flag's help)."""
    if flag == "auto":
        return fixed_ratio is not None or topology == "double_ring"
    return flag == "on"


def native_gpu(dev) -> bool:
    """The native extension serves this device (what the static engine needs)."""
    from .ops import _ext

    return dev.type == "cuda" and _ext.use_native(torch.empty(0, device=dev))


def weights_digest(model) -> str:
    """sha256 over every state_dict entry (name, dtype, bytes): equal on two ranks exactly when
    their replicas are bitwise equal."""
    import hashlib

    h = hashlib.sha256()
    for k, v in model.state_dict().items():
        t = v.detach().cpu().contiguous()
        h.update(f"{k}:{t.dtype}:{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())   # (reshape: 0-dim BN counters too)
    return h.hexdigest()


def resolve_engine(args, model, dev, world: int) -> bool:
    """--engine auto|autograd|static -> run the static MLP engine?"""
    from .models.mlp import MLP

    why = None
    if not isinstance(model, MLP):
        why = f"--model {args.model} is not an MLP"
    elif not native_gpu(dev):
        why = "the static engine needs the native extension on a GPU"
    elif args.grad_comm_dtype != "fp32":
        why = "--grad_comm_dtype bf16 runs on the autograd path"
    elif args.legacy_gossip and args.sync_every == "step" and args.topology != "allreduce" and world > 1:
        # the static engine's grad_mix always applies the combine (no reference-Q2 mode)
        why = "--legacy_gossip runs on the autograd path"
    elif getattr(args, "clip_grad_norm", 0.0) > 0:
        # the static engine's wgrad-fused optimizer epilogue cannot wait for a whole-model norm
        why = "--clip_grad_norm runs on the autograd path"
    elif getattr(args, "optimizer", None) == "lars":
        # ... nor for a tensor's whole gradient
        why = "--optimizer lars runs on the autograd path"
    elif getattr(args, "optimizer", None) == "lamb":
        # ... nor for a tensor's whole Adam direction
        why = "--optimizer lamb runs on the autograd path"
    elif getattr(args, "optimizer", None) == "lion":
        # the static engine's wgrad-fused optimizer epilogue has SGD and Adam forms only
        why = "--optimizer lion runs on the autograd path"
    elif getattr(args, "label_smoothing", 0.0) > 0:
        # the static engine's head kernels compute the plain loss
        why = "--label_smoothing runs on the autograd path"
    elif getattr(args, "class_weights", "none") != "none":
        # ... and has no weighted form
        why = "--class_weights runs on the autograd path"
    elif getattr(args, "focal_gamma", 0.0) > 0:
        # ... nor a focal one
        why = "--focal_gamma runs on the autograd path"
    elif getattr(args, "ema_decay", 0.0) > 0:
        # the static engine's wgrad-fused optimizer epilogue has no averaging pass behind it
        why = "--ema_decay runs on the autograd path"
    elif getattr(args, "fedprox_mu", 0.0) > 0:
        # ... and streams no anchor
        why = "--fedprox_mu runs on the autograd path"
    elif getattr(args, "mixup", 0.0) > 0 or getattr(args, "cutmix", 0.0) > 0:
        # the static engine's head kernels take hard labels
        why = "--mixup / --cutmix runs on the autograd path"
    elif getattr(args, "lr_schedule", "none") != "none":
        # the static engine's optimizer epilogue takes its rate from the host
        why = "--lr_schedule runs on the autograd path"
    elif getattr(args, "dropout", 0.0) > 0:
        # the static engine's layer chain has no pass between a layer's epilogue and the next GEMM
        why = "--dropout runs on the autograd path"
    elif getattr(args, "norm", "batch") == "group":
        # the static engine is a chain of GEMMs: it has no normalisation pass
        why = "--norm group runs on the autograd path"
    elif getattr(args, "norm", "batch") == "layer":
        why = "--norm layer runs on the autograd path"
    if args.engine == "static" and why is not None:
        raise SystemExit(f"--engine static: {why}")
    return args.engine != "autograd" and why is None


def schedule_from_args(args, default_total: int):
    """The optimizers' ``lr_schedule`` dict of the --lr_schedule flags (None: off), checked as the
    optimizers check it: a refusal exits naming the flags.  ``default_total`` stands in for an
    --lr_total_steps that was not given."""
    if args.lr_schedule == "none":
        return None
    from .optim import check_lr_schedule

    given = args.lr_total_steps is not None
    sched = dict(kind=args.lr_schedule, total_steps=int(args.lr_total_steps if given else default_total),
                 warmup_steps=args.warmup_steps, warmup_start=args.warmup_start, min_ratio=args.lr_min_ratio,
                 power=args.lr_power)
    try:
        return check_lr_schedule(sched)
    except ValueError as e:
        msg = str(e).replace("lr_schedule:", "--lr_schedule:").replace("total_steps", "--lr_total_steps") \
            .replace("warmup_steps", "--warmup_steps")
        if not given:
            msg += f" (--lr_total_steps was not given: the default horizon of this run is {default_total} steps)"
        raise SystemExit(msg)


def default_total_steps(args, n_batches: int, comm, world: int, dev) -> int:
    """The horizon --lr_total_steps defaults to: global epochs x local epochs x the steps one local
    epoch over the initial train loader runs.  Under per-step synchronisation on several ranks the
    shards, and so the loaders' lengths, differ between ranks, while every rank must run each
    lock-step update at the same rate: the ranks agree on the count the trainer will run (the
    shortest loader's, plus the one weighted tail step when a rank holds more), with the one
    all-reduce the trainer itself uses.  Under the global-epoch schedule each rank keeps its own."""
    if args.sync_every == "step" and world > 1:
        from .parallel.comm import MIN

        t = torch.tensor([float(n_batches), -float(n_batches)], device=dev)
        comm.all_reduce(t, MIN)
        lo, hi = int(t[0].item()), -int(t[1].item())
        n_batches = lo + (1 if hi > lo else 0)
    return args.epochs_global * args.epochs_local * n_batches


def main(argv=None):
    args = build_parser().parse_args(argv)
    # (the flags' own limits, before any process group or data exists; the default horizon comes later)
    schedule_from_args(args, max(args.warmup_steps, 0) + 1)
    if not 0.0 <= args.label_smoothing <= 1.0:
        raise SystemExit(f"--label_smoothing must be in [0, 1], got {args.label_smoothing}")
    from .data.class_weights import class_weights_from_labels, parse_class_weights
    try:
        class_weights = parse_class_weights(args.class_weights)   # (the list's length: once the dataset is known)
    except ValueError as e:
        raise SystemExit(str(e))
    if not (args.focal_gamma >= 0.0 and math.isfinite(args.focal_gamma)):
        raise SystemExit(f"--focal_gamma must be finite and >= 0, got {args.focal_gamma}")
    if args.focal_gamma > 0:
        for flag, v in (("--label_smoothing", args.label_smoothing), ("--mixup", args.mixup),
                        ("--cutmix", args.cutmix)):
            if v > 0:
                raise SystemExit(f"--focal_gamma with {flag}: there is no agreed focal loss over smoothed or "
                                 "class-probability targets; drop one of the two")
    if not 0.0 <= args.ema_decay < 1.0:
        raise SystemExit(f"--ema_decay must be in [0, 1), got {args.ema_decay}")
    if not (args.fedprox_mu >= 0.0 and math.isfinite(args.fedprox_mu)):
        raise SystemExit(f"--fedprox_mu must be finite and >= 0, got {args.fedprox_mu}")
    if args.fedprox_mu > 0:
        if args.optimizer in ("lars", "lamb"):
            raise SystemExit(f"--fedprox_mu with --optimizer {args.optimizer}: the trust ratios are defined on "
                             "g + weight_decay * w, there is no agreed form with a proximal term; use sgd, adam, "
                             "adamw or lion")
        if args.engine == "static":
            raise SystemExit("--engine static: --fedprox_mu runs on the autograd path")
    if not 0.0 <= args.dropout < 1.0:
        raise SystemExit(f"--dropout must be in [0, 1), got {args.dropout}")
    for flag, v in (("--mixup", args.mixup), ("--cutmix", args.cutmix)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise SystemExit(f"{flag} must be a finite alpha >= 0, got {v}")
    for flag, v in (("--mix_prob", args.mix_prob), ("--mix_switch_prob", args.mix_switch_prob)):
        if not 0.0 <= v <= 1.0:
            raise SystemExit(f"{flag} must be in [0, 1], got {v}")
    from .models import LAYER_NORM_MODELS, NORM_MODELS
    if args.norm == "layer" and args.model not in LAYER_NORM_MODELS:
        raise SystemExit(f"--norm layer: LayerNorm is built for the MLPs ({', '.join(LAYER_NORM_MODELS)}), "
                         f"not for --model {args.model}")
    if args.norm == "group" and args.model not in NORM_MODELS:
        raise SystemExit(f"--norm group: --model {args.model} has no normalisation layer "
                         f"(models with one: {', '.join(NORM_MODELS)})")
    if args.norm == "group" and args.gn_groups < 1:
        raise SystemExit(f"--gn_groups must be >= 1, got {args.gn_groups}")
    from . import prepare
    from .data.loader import get_loaders
    from .data.mix import BatchMix
    from .models import CrossEntropyLoss, FocalLoss, WeightedCrossEntropyLoss, build_model, dataset_for, xavier_init
    from .optim import StepLR, build_optimizer
    from .parallel.comm import default_comm
    from .parallel.ddp import DataParallel
    from .train.trainer import ema_eval, train_global
    from .train.validator import evaluate
    from .utils import distributed as D
    from .utils.checkpoint import Checkpointer, load_checkpoint
    from .utils.metrics import MetricsLogger

    backend = None if args.backend in ("auto", "mpi") else args.backend
    ctx = D.setup(backend, timeout_s=args.timeout, device=None if args.device == "auto" else args.device)
    rank, world = ctx.rank, ctx.world_size
    dev = ctx.device
    torch.manual_seed(args.seed)
    comm = default_comm(args.oneshot_bytes)

    dataset = args.dataset or dataset_for(args.model)
    if class_weights is not None and not isinstance(class_weights, str):
        from .data.datasets import CLASSES
        try:
            parse_class_weights(args.class_weights, CLASSES.get(dataset))
        except ValueError as e:
            raise SystemExit(str(e))
    try:
        model = build_model(args.model, dropout=args.dropout, norm=args.norm, gn_groups=args.gn_groups)
    except ValueError as e:   # (a --gn_groups that does not divide a width)
        raise SystemExit(str(e))
    xavier_init(model)
    use_engine = resolve_engine(args, model, dev, world)
    if use_engine:
        from .train.engine_adapter import build_engine

        step_dp = args.sync_every == "step" and world > 1
        hops = {"allreduce": 0, "ring": 1, "double_ring": 2}[args.topology]
        lw = args.local_weight if args.aggregation_type == "weighted" else None
        net, optimizer = build_engine(model.to(dev), args.batch_size, args.optimizer, args.lr, dev,
                                      momentum=args.momentum, weight_decay=args.weight_decay,
                                      world_size=world if step_dp else 1, use_graphs=True,
                                      bucket_cap_elems=int(args.bucket_mb * (1 << 20)) // 4,
                                      grad_mix=(hops, lw) if step_dp else None)
        flat = net.engine.flat
    else:
        flat = prepare(model, dev)
    fixed_ratio = args.fixed_ratio
    if args.partition == "skewed" and fixed_ratio is None:
        fixed_ratio = 0.5
    if args.partition == "balanced":
        fixed_ratio = None

    replace = resolve_replace(args.replace, fixed_ratio, args.topology)

    dp = None
    if use_engine:   # the engine synchronises its own gradients (per-step DP) or is a plain replica
        D.broadcast_module(model)
        flat.refresh_shadow()
    elif args.sync_every == "step" and world > 1:
        # (--grad_comm_dtype bf16: all-reduce / reduce-scatter buckets and the gossip exchange travel
        # as bf16 copies of the fp32 gradient)
        weighted = args.aggregation_type == "weighted"
        gossip = {"allreduce": 0, "ring": 1, "double_ring": 2}[args.topology]
        if args.shard_optimizer == "on" and (weighted or gossip):
            raise SystemExit("--shard_optimizer on needs --topology allreduce --aggregation_type equal (the "
                             "weighted mix and gossip give every rank its own update)")
        shard = not weighted and not gossip and (args.shard_optimizer == "on" or (args.shard_optimizer == "auto"
                                                                                   and dev.type == "cuda"))
        dp = DataParallel(model, comm, bucket_cap_mb=args.bucket_mb,
                          local_weight=args.local_weight if weighted else None,
                          comm_dtype=torch.bfloat16 if args.grad_comm_dtype == "bf16" else None,
                          shard_optimizer=shard, gossip=gossip, legacy_gossip=args.legacy_gossip)
        flat = dp.flat   # (sharding re-lays the flat buffers out)
    else:  # reference A6: broadcast every state_dict entry from rank 0
        D.broadcast_module(model)
        flat.refresh_shadow()
    if not use_engine:
        net = dp if dp is not None else model

    dtype = torch.bfloat16 if (args.dtype == "bf16" and dev.type == "cuda") else torch.float32
    # (the train loader fills in its dataset's class count)
    mix = (BatchMix(args.mixup, args.cutmix, args.mix_prob, args.mix_switch_prob)
           if args.mixup > 0 or args.cutmix > 0 else None)
    loaders = get_loaders(args.batch_size, world, rank, net, dev, fixed_ratio, dataset=dataset, comm=comm,
                          seed=args.seed, partition_rule=args.partition_rule, n_train=args.n_train,
                          n_test=args.n_test, dtype=dtype, augment=args.augment, data_root=args.data_root,
                          augment_val=args.augment_val, mix=mix)
    train_loader, val_loader, test_loader, trainset, valset, tr_idx, va_idx = loaders[:7]
    fixed_classes = loaders[7] if len(loaders) > 7 else None

    if class_weights is None:
        criterion = (FocalLoss(gamma=args.focal_gamma) if args.focal_gamma > 0
                     else CrossEntropyLoss(label_smoothing=args.label_smoothing))
    else:
        try:   # (a list: checked against the dataset's own class count)
            w0 = (class_weights_from_labels(trainset.targets[tr_idx], trainset.num_classes, class_weights)
                  if isinstance(class_weights, str) else parse_class_weights(args.class_weights, trainset.num_classes))
        except ValueError as e:
            raise SystemExit(str(e))
        # the buffer lives on the training device from here on: the step graphs bake its address in,
        # train_global rewrites its values in place (balanced / sqrt) at every global epoch
        criterion = (FocalLoss(gamma=args.focal_gamma, weight=torch.from_numpy(w0)).to(dev) if args.focal_gamma > 0
                     else WeightedCrossEntropyLoss(weight=torch.from_numpy(w0),
                                                   label_smoothing=args.label_smoothing).to(dev))
    if not use_engine:
        lr_schedule = None
        if args.lr_schedule != "none":    # (every rank enters: the default horizon may take a collective)
            lr_schedule = schedule_from_args(args, default_total_steps(args, len(train_loader), comm, world, dev))
        if lr_schedule is not None and not args.quiet:
            print(f"[rank {rank}] lr schedule {lr_schedule}")
        optimizer = build_optimizer(args.optimizer, model.parameters(), args.lr, args.momentum, args.weight_decay,
                                    max_grad_norm=args.clip_grad_norm if args.clip_grad_norm > 0 else None,
                                    ema_decay=args.ema_decay if args.ema_decay > 0 else None,
                                    ema_warmup=not args.ema_no_warmup, lr_schedule=lr_schedule,
                                    prox_mu=args.fedprox_mu if args.fedprox_mu > 0 else None,
                                    **(dict(lars_trust=args.lars_trust, lars_eps=args.lars_eps,
                                            lars_exclude_1d=not args.lars_adapt_1d)
                                       if args.optimizer == "lars" else
                                       dict(lamb_exclude_1d=not args.lamb_adapt_1d)
                                       if args.optimizer == "lamb" else {}))
    scheduler = StepLR(optimizer, step_size=args.step_size, gamma=args.gamma)

    os.makedirs(args.out_dir, exist_ok=True)
    logger = MetricsLogger(os.path.join(args.out_dir, "metrics.jsonl"), rank)
    logger.log(kind="config", world_size=world, pg_backend=ctx.backend, resolved_device=str(dev),
               resolved_engine="static" if use_engine else "autograd", **vars(args))
    per_rank = args.topology != "allreduce" or args.sync_every == "global_epoch"
    ckpt = Checkpointer(os.path.join(args.out_dir, "ckpt"), rank, per_rank=per_rank,
                        every=args.checkpoint_every) if args.checkpoint_every > 0 else None
    start, hist, rng_state = 0, None, None
    if args.resume:
        path = args.resume
        if path == "latest":
            path = Checkpointer(os.path.join(args.out_dir, "ckpt"), rank, per_rank=per_rank).latest()
        if path:
            sd = load_checkpoint(path, net if use_engine else model, optimizer, scheduler, rank=rank)
            flat.refresh_shadow()
            start, hist = sd["global_epoch"], sd["histories"]
            ex = sd.get("extra", {})
            rng_state = ex.get("rng_state")
            if "indices_train" in ex:
                from .data.loader import DeviceLoader
                from .train.trainer import loader_seed

                tr_idx, va_idx = ex["indices_train"].numpy(), ex["indices_val"].numpy()
                train_loader = DeviceLoader(trainset, tr_idx, args.batch_size, dev, dtype=dtype, augment=args.augment,
                                            seed=loader_seed(args.seed, rank, start), mix=mix)
                val_loader = DeviceLoader(valset, va_idx, args.batch_size, dev, dtype=dtype,
                                          augment=args.augment if args.augment_val else False,
                                          seed=(loader_seed(args.seed, rank, start) * 31 + 7) & 0x7FFFFFFF)
            if ex.get("fixed_classes") is not None:
                fc = ex["fixed_classes"]
                fixed_classes = fc.tolist() if torch.is_tensor(fc) else list(fc)

    from .utils import tracing

    timer = None
    if args.trace:
        tracing.enable(True)
        timer = tracing.PhaseTimer(dev, enabled=True)
    timelimit = args.time_limit if args.time_limit and args.time_limit > 0 else math.inf
    histories = train_global(
        net, train_loader, val_loader, trainset, valset, tr_idx, va_idx, criterion, optimizer, scheduler, dev, rank,
        world, args.epochs_local, args.epochs_global, timelimit, args.batch_size, args.prev_fraction,
        args.next_fraction, args.local_weight, args.aggregation_type, args.aggregation_by, comm=comm,
        topology=args.topology, fixed_classes=fixed_classes, fixed_ratio=fixed_ratio, sync_every=args.sync_every,
        dp=dp, partition_rule=args.partition_rule, repartition=not args.no_repartition, replace=replace,
        seed=args.seed, legacy_gossip=args.legacy_gossip, average_buffers=args.average_buffers,
        check_every=args.check_every, progress=not args.quiet, logger=logger, checkpointer=ckpt,
        start_global_epoch=start, histories=hist, dtype=dtype, verbose=not args.quiet, timer=timer,
        graphs=args.graphs, rng_state=rng_state, ref_samples_per_s=args.ref_samples_per_s,
        class_weights=class_weights)
    if timer is not None:
        phases = timer.summary()
        logger.log(kind="phase_times", phases=phases)
        if not args.quiet:
            for k, v in sorted(phases.items(), key=lambda kv: -kv[1]["total_ms"]):
                print(f"[rank {rank}] {k:10s} {v['total_ms']:10.2f} ms total  {v['mean_ms']:8.3f} ms x {v['count']}")

    if args.log_weights_digest:
        # this rank's final replica as a digest in its own metrics file (train_global left the
        # master whole)
        logger.log(kind="final_weights", sha256=weights_digest(model))
    result = {"histories": [list(h) if not isinstance(h, list) else h for h in histories]}
    if rank == 0 and not args.no_eval:
        # (--ema_decay: the test runs on the averaged weights, like every validation; train_global
        # left master and average whole)
        with ema_eval(optimizer):
            loss, acc, _, _ = evaluate(net, test_loader, criterion, dev, rank, num_classes=trainset.num_classes,
                                       verbose=not args.quiet)
        rep = {k: v for k, v in evaluate.last_report.items() if k != "confusion_matrix"}
        result.update(test_loss=loss, test_acc=acc, **rep)
        logger.log(kind="test", test_loss=loss, test_acc=acc, **rep)
    if rank == 0 and args.plots:
        from .utils.viz import plot_all

        plot_all(histories, args.epochs_global, args.epochs_local, 0, args.plots)
    if rank == 0:
        with open(os.path.join(args.out_dir, "histories.json"), "w") as f:
            json.dump(result, f)
    logger.close()
    D.teardown(ctx)
    return result


if __name__ == "__main__":
    main()
