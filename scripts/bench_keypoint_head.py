"""Device time of the keypoint-head kernels against the plain torch composition of the same functions, same process:
decode at R = 100, K = 17, S = 56 (boxes drawn like detections on a 1344 x 800 image), loss forward + backward at
N = 256 in fp32 and bf16, with the achieved fraction of HBM peak (8.0 TB/s) on the compulsory bytes.  One JSON line per
measurement; `--out FILE` also writes them there."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd import _C  # noqa: E402
from detectron2_amd.modeling import keypoint_rcnn_loss_from_targets  # noqa: E402
from detectron2_amd.structures import heatmaps_to_keypoints  # noqa: E402
from scripts.microbench import timeit  # noqa: E402

HBM_PEAK = 8.0e12


def graph_time(fn, inner=20, rep=10):
    """ms per call of `fn` with `inner` calls captured into one graph: device time, no host launch cost in the window."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return timeit(g.replay, rep=rep) / inner


def torch_decode(maps, rois):
    """The per-ROI composition the kernel replaces: resize, max / argmax, pool-resolution normaliser."""
    w, h = (rois[:, 2] - rois[:, 0]).clamp(min=1), (rois[:, 3] - rois[:, 1]).clamp(min=1)
    wc, hc = w.ceil(), h.ceil()
    out = maps.new_zeros(maps.shape[0], maps.shape[1], 4)
    for i in range(maps.shape[0]):
        size = (int(hc[i]), int(wc[i]))
        up = F.interpolate(maps[i:i + 1], size=size, mode="bicubic", align_corners=False)[0].flatten(1)
        top, pos = up.max(dim=1)
        out[i, :, 0] = ((pos % size[1]).float() + 0.5) * (w[i] / wc[i]) + rois[i, 0]
        out[i, :, 1] = ((pos // size[1]).float() + 0.5) * (h[i] / hc[i]) + rois[i, 1]
        out[i, :, 2] = top
        out[i, :, 3] = 1 / (maps[i].flatten(1) - top[:, None]).exp().sum(dim=1)
    return out


def torch_loss(logits, tgt, valid):
    rows = valid.view(-1).nonzero()[:, 0]
    x = logits.view(-1, logits.shape[2] * logits.shape[3])
    return F.cross_entropy(x[rows], tgt.view(-1)[rows], reduction="sum") / rows.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rep", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keypoint_head: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    res = []

    def emit(**kw):
        res.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- decode
    R, K, S = 100, 17, 56
    s = torch.exp(torch.empty(R).uniform_(math.log(32), math.log(500), generator=g))
    ar = torch.exp(torch.empty(R).uniform_(math.log(0.4), math.log(1.2), generator=g))  # (people: taller than wide)
    w, h = s * ar.sqrt(), s / ar.sqrt()
    cx, cy = torch.empty(R).uniform_(0, 1344, generator=g), torch.empty(R).uniform_(0, 800, generator=g)
    rois = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).to(dev)
    for dt in (torch.float32, torch.bfloat16):
        maps = (3 * torch.randn(R, K, S, S, generator=g)).to(dev).to(dt)
        ours, ref = heatmaps_to_keypoints(maps, rois).float(), torch_decode(maps.float(), rois)
        t_k = graph_time(lambda: heatmaps_to_keypoints(maps, rois))
        t_t = timeit(lambda: torch_decode(maps, rois), rep=5, warm=1) if dt == torch.float32 else None
        emit(op="heatmaps_to_keypoints", R=R, K=K, S=S, dtype=str(dt), kernel_us=t_k * 1e3,
             torch_loop_us=None if t_t is None else t_t * 1e3, output_pixels=int((w.ceil() * h.ceil()).sum()) * K,
             max_abs_diff_vs_torch_fp32_input=float((ours - ref).abs().max()) if dt == torch.float32 else None)

    # ---- loss forward + backward
    N = 256
    xy = torch.rand(N, 2, generator=g) * 600
    boxes = torch.cat([xy, xy + 20 + torch.rand(N, 2, generator=g) * 300], 1)
    kp = torch.cat([boxes[:, None, :2] + torch.rand(N, K, 2, generator=g) * (boxes[:, None, 2:] - boxes[:, None, :2]),
                    torch.randint(1, 3, (N, K, 1), generator=g).float()], 2)  # every row counts: the compulsory bytes
    boxes, kp = boxes.to(dev), kp.to(dev)
    from detectron2_amd.structures import Keypoints

    tgt, valid = Keypoints(kp).to_heatmap(boxes, S)
    L = _C.lib()
    one = torch.ones((), device=dev)
    for dt in (torch.float32, torch.bfloat16):
        x = (3 * torch.randn(N, K, S, S, generator=g)).to(dev).to(dt).requires_grad_(True)
        xd = x.detach()
        nbytes = xd.numel() * xd.element_size()
        ws_bytes = L.d2amd_keypoint_rcnn_loss_workspace_bytes(N * K)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss, stats = torch.empty((), device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        grad = torch.empty_like(xd)
        fwd = lambda: L.d2amd_keypoint_rcnn_loss_forward(_C.ptr(xd), _C.ptr(kp), _C.ptr(boxes), N, K, S, _C.dtype_code(xd),
                                                         0.0, _C.ptr(loss), _C.ptr(stats), _C.ptr(ws), ws_bytes, _C.stream())
        bwd = lambda: L.d2amd_keypoint_rcnn_loss_backward(_C.ptr(xd), _C.ptr(ws), _C.ptr(one), N, K, S, _C.dtype_code(xd),
                                                          0.0, _C.ptr(grad), _C.stream())
        assert fwd() == 0 and bwd() == 0
        t_f, t_b = graph_time(fwd), graph_time(bwd)

        def ours():
            l, _ = keypoint_rcnn_loss_from_targets(x, kp, boxes)
            l.backward()
            x.grad = None

        def theirs():
            torch_loss(x, tgt, valid).backward()
            x.grad = None

        t_o, t_t = timeit(ours, rep=args.rep), timeit(theirs, rep=args.rep)
        want = torch_loss(xd.double(), tgt, valid)
        emit(op="keypoint_rcnn_loss", N=N, K=K, S=S, dtype=str(dt), valid_rows=int(stats[0]),
             forward_kernels_us=t_f * 1e3, backward_kernel_us=t_b * 1e3, forward_backward_autograd_us=t_o * 1e3,
             torch_forward_backward_us=t_t * 1e3, forward_bytes=nbytes, backward_bytes=2 * nbytes,
             forward_frac_hbm_peak=nbytes / (t_f * 1e-3) / HBM_PEAK, backward_frac_hbm_peak=2 * nbytes / (t_b * 1e-3) / HBM_PEAK,
             loss_rel_err_vs_float64=float((loss.double() - want).abs() / want))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
