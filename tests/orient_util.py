"""Shared by tests/test_orient_ingest.py and tests/test_gpu_orient_ingest.py: the orientation rule of include/pv_mi355x.h
written out index by index -- independently of `transforms.oriented`, which the tests check against it -- and the dense,
pre-oriented copies of videos that are the oracle of an oriented record: the same launch with orient = 0 on such a copy
writes the same bits."""
import torch

import yuv16_util as Y16
import yuv_util as YU

CODES = tuple(range(8))


def displayed_size(hs, ws, orient):
    return (ws, hs) if orient & 1 else (hs, ws)


def stored_index(y, x, hs, ws, orient):
    """(row, column) of the stored pixel that displayed pixel (y, x) shows: the table of the header."""
    rot, mirror = orient & 3, orient >> 2
    wd = displayed_size(hs, ws, orient)[1]
    xp = wd - 1 - x if mirror else x
    return [(y, xp), (hs - 1 - xp, y), (hs - 1 - y, ws - 1 - xp), (xp, ws - 1 - y)][rot]


def by_index(plane, orient):
    """The displayed frame of a 2-d stored `plane`, pixel by pixel through `stored_index`."""
    hs, ws = plane.shape
    hd, wd = displayed_size(hs, ws, orient)
    out = torch.empty((hd, wd), dtype=plane.dtype)
    for y in range(hd):
        for x in range(wd):
            out[y, x] = plane[stored_index(y, x, hs, ws, orient)]
    return out


def turned(x, orient):
    """`torch.rot90` / `flip` over the last two dimensions, dense: the pre-oriented copy of planes or of a [.., H, W] video."""
    x = torch.rot90(x, -(orient & 3), (-2, -1))
    return (x.flip(-1) if orient & 4 else x).contiguous()


def upsampled(c):
    """A chroma plane replicated over its 2 x 2 luma blocks."""
    return c.repeat_interleave(2, -2).repeat_interleave(2, -1)


def yuv_preoriented(y, u, v, layout, orient):
    """The Y, U and V planes oriented SEPARATELY, then repacked as `layout` frames at pitch W with no coded padding: the
    [N, Hd*3/2, Wd] video a caller would have had to build, as the `Packed` of yuv_util / yuv16_util (`.frames(device)`)."""
    planes = [turned(p, orient) for p in (y, u, v)]
    if layout in Y16.INTERLEAVED + Y16.PLANAR:
        return Y16.pack(*planes, layout)
    return YU.pack(*planes, layout)
