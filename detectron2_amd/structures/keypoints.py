"""`detectron2.structures.keypoints` on the hot path: `Keypoints` (keypoints.py:8-101) whose `to_heatmap` is one
elementwise launch (csrc/keypoint_head.hip, bit-identical to the reference's ~25 fp32 ops), and `heatmaps_to_keypoints`
(keypoints.py:165-235) as ONE launch for all ROIs with no host read -- the reference loops over the ROIs in Python with
two host reads, a bicubic `F.interpolate` and a synchronising assert each."""
from typing import Any, List, Tuple, Union

import numpy as np
import torch

from .. import _C

__all__ = ["Keypoints", "heatmaps_to_keypoints", "heatmaps_to_keypoints_fp32"]


def _keypoints_to_heatmap(keypoints: torch.Tensor, rois: torch.Tensor, heatmap_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _C.require_gpu(keypoints, rois, op="Keypoints.to_heatmap")
    if rois.numel() == 0:
        return rois.new().long(), rois.new().long()
    n, k = keypoints.shape[:2]
    assert rois.shape == (n, 4), (rois.shape, keypoints.shape)
    kp = keypoints.detach().to(dtype=torch.float32).contiguous()
    r = rois.detach().to(device=kp.device, dtype=torch.float32).contiguous()
    heatmaps = torch.empty((n, k), dtype=torch.int64, device=kp.device)
    valid = torch.empty((n, k), dtype=torch.int64, device=kp.device)
    with _C.on_device(kp.device):
        _C.check(_C.lib().d2amd_keypoints_to_heatmap(_C.ptr(kp), _C.ptr(r), n, k, int(heatmap_size), _C.ptr(heatmaps),
                                                     _C.ptr(valid), _C.stream()))
    return heatmaps, valid


class Keypoints:
    """(N, K, 3) keypoint annotations: x, y, visibility (0 = not labelled, 1 = labelled, 2 = labelled and visible)."""

    def __init__(self, keypoints: Union[torch.Tensor, np.ndarray, List[List[float]]]):
        device = keypoints.device if isinstance(keypoints, torch.Tensor) else torch.device("cpu")
        keypoints = torch.as_tensor(keypoints, dtype=torch.float32, device=device)
        assert keypoints.dim() == 3 and keypoints.shape[2] == 3, keypoints.shape
        self.tensor = keypoints

    def __len__(self) -> int:
        return self.tensor.size(0)

    def to(self, *args: Any, **kwargs: Any) -> "Keypoints":
        return type(self)(self.tensor.to(*args, **kwargs))

    @property
    def device(self) -> torch.device:
        return self.tensor.device

    def to_heatmap(self, boxes: torch.Tensor, heatmap_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (heatmaps int64 (N, K): the cell y * heatmap_size + x of every keypoint in its box, 0 where it does not
        count; valid int64 (N, K)).  Rows of a box of zero extent (an undefined integer cast in the reference) are
        invalid."""
        return _keypoints_to_heatmap(self.tensor, boxes, heatmap_size)

    def __getitem__(self, item: Union[int, slice, torch.BoolTensor]) -> "Keypoints":
        if isinstance(item, int):
            return Keypoints(self.tensor[item][None])
        return Keypoints(self.tensor[item])

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(num_instances={len(self.tensor)})"

    @staticmethod
    def cat(keypoints_list: List["Keypoints"]) -> "Keypoints":
        assert isinstance(keypoints_list, (list, tuple)) and len(keypoints_list) > 0
        assert all(isinstance(k, Keypoints) for k in keypoints_list)
        return type(keypoints_list[0])(torch.cat([k.tensor for k in keypoints_list], dim=0))


def heatmaps_to_keypoints_fp32(maps: torch.Tensor, rois: torch.Tensor, return_pos: bool = False):
    """The kernel's own results: (R, K, 4) fp32 (x, y, logit, score) whatever `maps.dtype` is and, with `return_pos`,
    the (R, K) int32 linear index y * W' + x of the maximum in the ROI-sized map (the lowest among exact ties)."""
    _C.require_gpu(maps, rois, op="heatmaps_to_keypoints")
    assert maps.dim() == 4 and maps.size(2) == maps.size(3), maps.shape
    r, k, s = maps.shape[:3]
    assert rois.shape == (r, 4), (rois.shape, maps.shape)
    x = maps.detach().contiguous()
    b = rois.detach().to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty((r, k, 4), dtype=torch.float32, device=x.device)
    pos = torch.empty((r, k), dtype=torch.int32, device=x.device) if return_pos else None
    with _C.on_device(x.device):
        _C.check(_C.lib().d2amd_heatmaps_to_keypoints(_C.ptr(x), _C.ptr(b), r, k, s, _C.dtype_code(x), _C.ptr(out),
                                                      _C.ptr(pos), _C.stream()))
    return (out, pos) if return_pos else out


def heatmaps_to_keypoints(maps: torch.Tensor, rois: torch.Tensor) -> torch.Tensor:
    """(R, K, S, S) heatmaps of logits + (R, 4) boxes -> (R, K, 4) = (x, y, logit, score) in `maps.dtype`."""
    return heatmaps_to_keypoints_fp32(maps, rois).to(maps.dtype)
