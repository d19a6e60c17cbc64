"""Device time of the fused box-head loss (csrc/box_loss.hip) against the same loss composed from torch ops the way the
reference composes it (fast_rcnn.py:88-115 statistics with their four nonzero() reads, cross_entropy or the one-hot
sigmoid BCE, :424-463 nonzero + two-level gather + get_deltas + smooth-L1, autograd), forward + backward, alternating in
one process.  Shapes: R = 1024, K = 80 (Mask R-CNN, 2 images) with softmax; R = 8192, K = 1203 (LVIS heads) with softmax
and with the sigmoid loss; class-specific deltas, bf16, a quarter of the rows foreground, no padding (the composition
has no notion of it).  Per side: median of `--rounds` windows of about `--window` seconds, kernel launches of one
forward + backward (torch.profiler) and host synchronisations (torch's sync debug mode).  Also the compulsory bytes
(scores read twice and written once, deltas' gradient written once) and the share of HBM peak (8.0 TB/s) the fused side
reaches on them.  One JSON line per shape; `--out FILE` also writes them there."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd.modeling import fast_rcnn_losses_with_stats  # noqa: E402

HBM_PEAK = 8.0e12
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SHAPES = [(1024, 80, False), (8192, 1203, False), (8192, 1203, True)]


def composed(scores, deltas, classes, boxes, gt, K, sigmoid):
    pred = scores.argmax(dim=1)  # _log_classification_stats
    fg = (classes >= 0) & (classes < K)
    num_fg = fg.nonzero().numel()
    fg_gt, fg_pred = classes[fg], pred[fg]
    counts = (num_fg, (fg_pred == K).nonzero().numel(), (pred == classes).nonzero().numel(),
              (fg_pred == fg_gt).nonzero().numel())
    if sigmoid:  # sigmoid_cross_entropy_loss
        n = scores.shape[0]
        target = scores.new_zeros(n, K + 1)
        target[torch.arange(n, device=scores.device), classes] = 1
        cls = F.binary_cross_entropy_with_logits(scores[:, :-1], target[:, :K], reduction="none").sum() / n
    else:
        cls = F.cross_entropy(scores, classes, reduction="mean")
    idx = fg.nonzero(as_tuple=True)[0]  # box_reg_loss
    d = deltas.view(-1, K, 4)[idx, classes[idx]]
    pb, gb = boxes[idx], gt[idx]
    w, h = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
    cx, cy = pb[:, 0] + 0.5 * w, pb[:, 1] + 0.5 * h
    tw, th = gb[:, 2] - gb[:, 0], gb[:, 3] - gb[:, 1]
    wx, wy, ww, wh = WEIGHTS
    tgt = torch.stack([wx * (gb[:, 0] + 0.5 * tw - cx) / w, wy * (gb[:, 1] + 0.5 * th - cy) / h, ww * torch.log(tw / w),
                       wh * torch.log(th / h)], dim=1)
    box = (d - tgt).abs().sum() / max(classes.numel(), 1.0)
    return cls, box, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timing window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev, lines = "cuda", []
    for R, K, sigmoid in SHAPES:
        g = torch.Generator().manual_seed(0)
        classes = torch.where(torch.rand(R, generator=g) < 0.25, torch.randint(0, K, (R,), generator=g), K).to(dev)
        xy, wh = 800 * torch.rand(R, 2, generator=g), 16 + 300 * torch.rand(R, 2, generator=g)
        boxes = torch.cat([xy, xy + wh], dim=1).to(dev)
        gt = (boxes.cpu() + 0.1 * (torch.rand(R, 4, generator=g) - 0.5) * torch.cat([wh, wh], dim=1)).to(dev)
        scores = (2 * torch.randn(R, K + 1, generator=g)).to(dev, dtype).requires_grad_()
        deltas = (0.3 * torch.randn(R, 4 * K, generator=g)).to(dev, dtype).requires_grad_()

        def fused():
            losses, _ = fast_rcnn_losses_with_stats(scores, deltas, classes, boxes, gt, box2box_weights=WEIGHTS,
                                                    use_sigmoid_ce=sigmoid)
            (losses["loss_cls"] + losses["loss_box_reg"]).backward()

        def torch_ops():
            cls, box, _ = composed(scores, deltas, classes, boxes, gt, K, sigmoid)
            (cls + box).backward()

        def window(fn, reps):
            scores.grad = deltas.grad = None
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
                scores.grad = deltas.grad = None
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        def counts(fn):
            """(kernel launches, host synchronisations) of one forward + backward"""
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                fn()
            torch.cuda.set_sync_debug_mode("default")
            syncs = sum("synchroniz" in str(w.message) for w in seen)
            try:
                from torch.profiler import ProfilerActivity, profile

                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                launches = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name
                               and "emset" not in e.name)
            except Exception:  # (a build of torch without the device tracer)
                launches = None
            scores.grad = deltas.grad = None
            return launches, syncs

        sides = {"fused": fused, "composed": torch_ops}
        reps, times, meta = {}, {"fused": [], "composed": []}, {}
        for name, fn in sides.items():  # warm-up, and repetitions that fill the window
            window(fn, 3)
            reps[name] = max(5, int(a.window * 1e3 / window(fn, 5)) + 1)
        for _ in range(a.rounds):  # alternating
            for name, fn in sides.items():
                times[name].append(window(fn, reps[name]))
        for name, fn in sides.items():
            meta[name] = counts(fn)
        es = scores.element_size()
        nbytes = 3 * R * (K + 1) * es + R * 4 * K * es + R * (8 + 32 + 8)
        f_ms, c_ms = statistics.median(times["fused"]), statistics.median(times["composed"])
        res = {"bench": "box_loss", "device": torch.cuda.get_device_name(0), "rows": R, "classes": K,
               "cls_loss": "sigmoid" if sigmoid else "softmax", "dtype": a.dtype, "fused_fwd_bwd_ms": round(f_ms, 4),
               "composed_fwd_bwd_ms": round(c_ms, 4), "speedup": round(c_ms / f_ms, 2),
               "fused_windows_ms": [round(t, 4) for t in times["fused"]],
               "composed_windows_ms": [round(t, 4) for t in times["composed"]], "reps_per_window": reps,
               "fused_launches": meta["fused"][0], "fused_host_syncs": meta["fused"][1],
               "composed_launches": meta["composed"][0], "composed_host_syncs": meta["composed"][1],
               "compulsory_bytes": nbytes, "fused_share_of_hbm_peak": round(nbytes / (f_ms * 1e-3) / HBM_PEAK, 4)}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
