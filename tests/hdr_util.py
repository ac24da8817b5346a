"""Shared by tests/test_hdr_ingest.py and tests/test_gpu_hdr_ingest.py: the tap map of `pv_hdr_views` (include/pv_mi355x.h,
"HDR sources") restated from the standards, independently of `transforms.tone_params` / `transforms.hdr_to_sdr`, which the
tests check against it -- as tests/yuv16_util.py is independent of `transforms.yuv_geometry`.

Everything runs in the dtype it is asked for: float64 is the reference; float32 on the CPU (correctly rounded log / exp / pow /
division) is the fp32 floor of the formulas themselves, against which the device's error is measured (E32)."""
import math

import torch

# SMPTE ST 2084
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
# BT.2100 HLG
A = 0.17883277
B = 1.0 - 4.0 * A
C = 0.5 - A * math.log(4.0 * A)
LUMA = (0.2627, 0.6780, 0.0593)
# BT.2020's OETF with its continuous constants
BETA, ALPHA = 0.018053968510807, 1.09929682680944
BT2087 = [[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]]
IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
OFF = 3e38


def pq_eotf(e):
    """Display light in nits of a PQ signal e in [0, 1] (float64 tensor or float)."""
    e = torch.as_tensor(e, dtype=torch.float64)
    p = e ** (1.0 / M2)
    return 10000.0 * (torch.clamp(p - C1, min=0.0) / (C2 - C3 * p)) ** (1.0 / M1)


def pq_inverse_eotf(nits):
    """The PQ signal of `nits` of display light: the inverse of `pq_eotf`."""
    y = (torch.as_tensor(nits, dtype=torch.float64) / 10000.0) ** M1
    return ((C1 + C2 * y) / (1.0 + C3 * y)) ** M2


def hlg_inverse_oetf(e):
    """Scene light in [0, 1] of an HLG signal e in [0, 1]."""
    e = torch.as_tensor(e, dtype=torch.float64)
    return torch.where(e <= 0.5, e * e / 3.0, (torch.exp((e - C) / A) + B) / 12.0)


def mobius(m, j, peak):
    """ffmpeg's "mobius" curve on a light level m >= 0: the identity up to j, then a Moebius map that takes `peak` to 1."""
    m = torch.as_tensor(m, dtype=torch.float64)
    a = -j * j * (peak - 1.0) / (j * j - 2.0 * j + peak)
    b = (j * j - 2.0 * j * peak + peak) / (peak - 1.0)
    scale = (b * b + 2.0 * b * j + j * j) / (b - a)
    return torch.where(m > j, scale * (m + a) / (m + b), m)


def oetf(lin):
    lin = torch.as_tensor(lin, dtype=torch.float64)
    return torch.where(lin < BETA, 4.5 * lin, ALPHA * lin ** 0.45 - (ALPHA - 1.0))


def tone(transfer, peak_nits=1000.0, white_nits=203.0, knee=0.3, curve=True, gamut=BT2087):
    """The 16 values of the header's `tone` table as Python floats (float64)."""
    p = peak_nits / white_nits
    head = [10000.0 / white_nits, 0.0] if transfer == "pq" else [p, 0.2 + 0.42 * math.log10(peak_nits / 1000.0)]
    if curve:
        j = knee
        a = -j * j * (p - 1.0) / (j * j - 2.0 * j + p)
        b = (j * j - 2.0 * j * p + p) / (p - 1.0)
        mid = [j, (b * b + 2.0 * b * j + j * j) / (b - a), a, b]
    else:
        mid = [OFF, 1.0, 0.0, 0.0]
    return head + mid + [g for row in gamut for g in row] + [0.0]


def to_sdr(rgb255, transfer, table, dtype=torch.float64):
    """Steps 1 to 4 of the header on [..., 3, H, W] taps in 0..255, channel by channel, every operation in `dtype`; `table` is
    the 16 tone values (any sequence or tensor), taken into `dtype` first."""
    t = [torch.tensor(float(v), dtype=dtype) for v in torch.as_tensor(table, dtype=torch.float64).reshape(-1).tolist()]
    k = lambda v: torch.tensor(v, dtype=dtype)                                         # noqa: E731
    x = torch.as_tensor(rgb255).to(dtype)
    e = [x[..., c, :, :] / k(255.0) for c in range(3)]
    if transfer == "pq":
        lin = []
        for c in range(3):
            p = torch.pow(e[c], k(1.0 / M2))
            q = torch.clamp(p - k(C1), min=0.0) / (k(C2) - k(C3) * p)
            lin.append(torch.pow(q, k(1.0 / M1)) * t[0])
    else:
        s = [torch.where(e[c] <= k(0.5), e[c] * e[c] / k(3.0), (torch.exp((e[c] - k(C)) / k(A)) + k(B)) / k(12.0)) for c in range(3)]
        ys = k(LUMA[0]) * s[0] + k(LUMA[1]) * s[1] + k(LUMA[2]) * s[2]
        pos = ys > 0
        gain = torch.where(pos, torch.pow(torch.where(pos, ys, torch.ones_like(ys)), t[1]) * t[0], torch.zeros_like(ys))
        lin = [s[c] * gain for c in range(3)]
    m = torch.maximum(torch.maximum(lin[0], lin[1]), lin[2])
    over = m > t[2]
    ms = torch.where(over, m, torch.ones_like(m))
    ratio = torch.where(over, t[3] * (ms + t[4]) / ((ms + t[5]) * ms), torch.ones_like(m))
    lin = [v * ratio for v in lin]
    out = []
    for c in range(3):
        g = torch.clamp(t[6 + 3 * c] * lin[0] + t[7 + 3 * c] * lin[1] + t[8 + 3 * c] * lin[2], 0.0, 1.0)
        v = torch.where(g < k(BETA), k(4.5) * g, k(ALPHA) * torch.pow(g, k(0.45)) - k(ALPHA - 1.0))
        out.append(k(255.0) * v)
    return torch.stack(out, dim=-3)


def rgb_taps(y, u, v, matrix, dtype=torch.float64):
    """clamp(M . (Y, U, V, 1), 0, 255) with chroma replicated over 2 x 2, straight from the codes, every operation in `dtype`
    (`matrix`: the fp32 values the device holds): [n, 3, hs, ws]."""
    up = [c.to(dtype).repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v)]
    m = matrix.float().to(dtype)
    out = [m[c, 0] * y.to(dtype) + m[c, 1] * up[0] + m[c, 2] * up[1] + m[c, 3] for c in range(3)]
    return torch.clamp(torch.stack(out, dim=1), 0.0, 255.0)
