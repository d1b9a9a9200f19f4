"""Host <-> device array helpers shared by the mask and keypoint GPU tests."""
import numpy as np
import torch


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def words(t):
    """a device tensor's bytes as uint32 on the host"""
    return t.cpu().numpy().view(np.uint32)


def bits(a):
    """a host array's bytes as uint32"""
    return np.ascontiguousarray(a).view(np.uint32)


def unpack(w, W):
    """uint32 [..., Wd] -> bool [..., W]"""
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=-1, bitorder='little')[..., :W].astype(bool)
