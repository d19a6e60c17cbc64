"""Device time of the fused semantic-segmentation head (csrc/sem_seg.hip) against the composition of torch ops the
reference runs, same GPU, same process: loss forward + backward of (2, 54, 200, 336) bf16 channels_last logits at
common_stride 4 -- the stride-4 map of the benchmark's 800 x 1344 images -- and the label decode to (800, 1344), with the
fused kernels' fraction of HBM peak (8.0 TB/s) on their compulsory bytes (logits + targets + lse, + the gradient in the
backward).  Results are compared at the timed size.  One JSON line per measurement; `--out FILE` also writes them."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_amd import _C  # noqa: E402
from detectron2_amd.modeling import sem_seg_labels, sem_seg_loss  # noqa: E402
from scripts.microbench import timeit  # noqa: E402

HBM_PEAK = 8.0e12


def torch_loss(x, t, s, ignore_value):  # semantic_seg.py:255-267
    up = F.interpolate(x.float(), scale_factor=s, mode="bilinear", align_corners=False)
    return F.cross_entropy(up, t, reduction="mean", ignore_index=ignore_value)


def torch_labels(x, s, image_size, output_size):  # semantic_seg.py:241-243, postprocessing.py:77-100, argmax
    up = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)
    out = []
    for r in up:
        r = r[:, :image_size[0], :image_size[1]].expand(1, -1, -1, -1)
        out.append(F.interpolate(r, size=output_size, mode="bilinear", align_corners=False)[0].argmax(dim=0))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rep", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=4, default=[2, 54, 200, 336], metavar=("N", "C", "h", "w"))
    ap.add_argument("--stride", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sem_seg_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    (N, C, h, w), s, ign = args.shape, args.stride, 255
    SH, SW = s * h, s * w
    res = []

    def emit(**kw):
        res.append(kw)
        print(json.dumps(kw), flush=True)

    x = (3 * torch.randn(N, C, h, w, generator=g)).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    xd = x.detach()
    # targets: regions of 32 x 32 pixels of one class (a segmentation map is piecewise constant), or i.i.d. pixels
    coarse = torch.randint(0, C, (N, -(-SH // 32), -(-SW // 32)), generator=g)
    coarse[torch.rand(coarse.shape, generator=g) < 0.1] = ign
    regions = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :SH, :SW].contiguous().to(dev)
    iid = torch.randint(0, C, (N, SH, SW), generator=g)
    iid[torch.rand(iid.shape, generator=g) < 0.1] = ign
    L = _C.lib()
    ws_bytes = L.d2amd_sem_seg_loss_workspace_bytes(N, h, w, s)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    loss, stats = torch.empty((), device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    grad, one = torch.empty_like(xd), torch.ones((), device=dev)
    logit_bytes, lse_bytes = xd.numel() * xd.element_size(), N * SH * SW * 4
    for name, t in (("regions", regions), ("iid", iid.to(dev))):
        fwd = lambda: L.d2amd_sem_seg_loss_forward(_C.ptr(xd), _C.ptr(t), N, C, h, w, s, _C.dtype_code(xd), _C.NHWC, ign,
                                                   _C.ptr(loss), _C.ptr(stats), _C.ptr(ws), ws_bytes, _C.stream())
        bwd = lambda: L.d2amd_sem_seg_loss_backward(_C.ptr(xd), _C.ptr(t), _C.ptr(ws), _C.ptr(one), N, C, h, w, s,
                                                    _C.dtype_code(xd), _C.NHWC, ign, _C.ptr(grad), _C.stream())
        assert fwd() == 0 and bwd() == 0
        t_f, t_b = timeit(fwd, rep=args.rep), timeit(bwd, rep=args.rep)

        def ours():
            sem_seg_loss(x, t, common_stride=s, ignore_value=ign).backward()
            g_, x.grad = x.grad, None
            return g_

        def theirs():
            torch_loss(x, t, s, ign).backward()
            g_, x.grad = x.grad, None
            return g_

        t_o, t_t = timeit(ours, rep=args.rep), timeit(theirs, rep=max(3, args.rep // 5))
        want = torch_loss(xd, t, s, ign)
        g_ours, g_theirs = ours().float(), theirs().float()
        f_bytes, b_bytes = logit_bytes + t.numel() * 8 + lse_bytes, 2 * logit_bytes + t.numel() * 8 + lse_bytes
        emit(op="sem_seg_loss", shape=[N, C, h, w], stride=s, dtype="bfloat16", layout="channels_last", targets=name,
             count=int(stats[0]), forward_kernels_us=t_f * 1e3, backward_kernel_us=t_b * 1e3,
             fused_forward_backward_autograd_us=t_o * 1e3, torch_forward_backward_us=t_t * 1e3,
             speedup=t_t / t_o, forward_bytes=f_bytes, backward_bytes=b_bytes,
             forward_frac_hbm_peak=f_bytes / (t_f * 1e-3) / HBM_PEAK, backward_frac_hbm_peak=b_bytes / (t_b * 1e-3) / HBM_PEAK,
             loss_rel_diff_vs_torch_fp32=float((loss - want).abs() / want),
             grad_max_diff_times_count=float((g_ours - g_theirs).abs().max()) * int(stats[0]),
             grad_max_times_count=float(g_theirs.abs().max()) * int(stats[0]))

    # ---- label decode to the padded image's size
    size = (SH, SW)
    ours_l = sem_seg_labels(xd, [size] * N, [size] * N, common_stride=s)
    ref_l = torch_labels(xd.float(), s, size, size)
    t_k = timeit(lambda: sem_seg_labels(xd, [size] * N, [size] * N, common_stride=s), rep=args.rep)
    t_t = timeit(lambda: torch_labels(xd, s, size, size), rep=max(3, args.rep // 5))
    l_bytes = logit_bytes + ours_l.numel() * 8
    emit(op="sem_seg_labels", shape=[N, C, h, w], stride=s, output=list(size), dtype="bfloat16", layout="channels_last",
         fused_us=t_k * 1e3, torch_us=t_t * 1e3, speedup=t_t / t_k, bytes=l_bytes,
         frac_hbm_peak=l_bytes / (t_k * 1e-3) / HBM_PEAK,
         labels_equal_to_torch_fp32=float((ours_l == ref_l).float().mean()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
