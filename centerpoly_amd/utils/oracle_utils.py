"""gen_oracle_map (reference: src/lib/utils/oracle_utils.py:8-42), the dense ground-truth head map of the
`--eval_oracle_*` switches, built on the device.

The reference floods the map breadth-first from the objects' centres on the host (numba) and copies the dense result
back; here it is one launch of `cp_oracle_map`, the fill's closed form (include/centerpoly_hip.h): every pixel takes the
feature row of the lowest-numbered seed at minimal L1 distance, a seed's own pixel the row of the last object centred
there, and an object is a seed when `ind > 0`.
"""
import torch

from .. import _C


def gen_oracle_map(feat, ind, w, h):
    """feat [B, M, D] float32, ind [B, M] int64 (device tensors) -> [B, D, h, w] float32 on the current stream."""
    if feat.dim() != 3 or ind.dim() != 2 or tuple(ind.shape) != tuple(feat.shape[:2]):
        raise ValueError("gen_oracle_map: feat [B, M, D] and ind [B, M] expected, got %s and %s"
                         % (tuple(feat.shape), tuple(ind.shape)))
    if feat.dtype != torch.float32 or ind.dtype != torch.int64:
        raise ValueError("gen_oracle_map: feat must be float32 and ind int64, got %s and %s" % (feat.dtype, ind.dtype))
    feat, ind = feat.detach().contiguous(), ind.contiguous()
    B, M, D = feat.shape
    pf, pi = _C.ptr(feat), _C.ptr(ind)                      # refuses host tensors
    out = torch.empty((B, D, int(h), int(w)), dtype=torch.float32, device=feat.device)
    _C.check(_C.lib().cp_oracle_map(pf, pi, B, M, D, int(h), int(w), _C.ptr(out), _C.stream()), "cp_oracle_map")
    return out
