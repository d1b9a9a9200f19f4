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


def dev_words(a, cuda):
    """host uint32 words -> the int32 device tensor the mask operators take"""
    return dev(np.ascontiguousarray(a).view(np.int32), cuda)


def host(out):
    """a dict of device tensors -> numpy"""
    return {k: v.cpu().numpy() for k, v in out.items()}


def pack(mask, H, Wd):
    """bool [h, w] -> uint32 [H, Wd], zero outside the image"""
    full = np.zeros((H, Wd * 32), dtype=np.uint8)
    full[:mask.shape[0], :mask.shape[1]] = mask
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(H, Wd)


def check_mask(got, r, want, where):
    """one mask of a mask_rle result against {'n_runs', 'counts', 'chars', 'area', 'bbox'}"""
    n = int(got['n_runs'][r])
    assert n == want['n_runs'], (where, n, want['n_runs'])
    assert np.array_equal(got['counts'][r, :n].view(np.uint32), want['counts']), where
    nb = int(got['n_bytes'][r])
    assert got['chars'][r, :nb].tobytes() == want['chars'], where
    assert int(got['area'][r].view(np.uint32)) == want['area'], where
    assert got['bbox'][r].view(np.uint32).tolist() == want['bbox'], (where, got['bbox'][r], want['bbox'])
