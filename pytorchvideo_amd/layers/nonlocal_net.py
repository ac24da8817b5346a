"""Non-local block (Wang et al., "Non-local Neural Networks", CVPR 2018), host mirror of the reference's
pytorchvideo/layers/nonlocal_net.py: same attribute names, construction order and state_dict keys
(`conv_theta`, `conv_phi`, `conv_g`, `conv_out`, `norm`), so reference checkpoints of the "NL" variants of
Slow / I3D / SlowFast load unchanged.

    y = x + norm(conv_out(A g(pool(x)))),   A = softmax(theta(x) phi(pool(x))^T / sqrt(dim_inner))    ("softmax")
                                            A = theta(x) phi(pool(x))^T / (number of pooled positions) ("dot_product")

over all T*H*W positions of a clip.  In a bf16 deploy plan the middle is one launch of pv_nonlocal_attention
(csrc/pv_nlattn.hip; emit.emit_nonlocal): the position x position matrix A is never stored.
"""
import torch
import torch.nn as nn

from .utils import set_attributes


class NonLocal(nn.Module):
    def __init__(self, *, conv_theta, conv_phi, conv_g, conv_out, pool=None, norm=None, instantiation="dot_product"):
        super().__init__()
        set_attributes(self, locals())
        assert None not in (conv_theta, conv_phi, conv_g, conv_out)
        assert instantiation in ("dot_product", "softmax"), "Unknown norm type {}".format(instantiation)
        widths = {conv_theta.out_channels, conv_phi.out_channels, conv_g.out_channels, conv_out.in_channels}
        assert len(widths) == 1, "Nonlocal convolution's input/ output dimension mismatch."

    def forward(self, x):
        ci = self.conv_theta.out_channels
        n, _, t, h, w = x.shape
        keys = x if self.pool is None else self.pool(x)
        theta = self.conv_theta(x).reshape(n, ci, -1)         # [n, ci, Nq]
        phi = self.conv_phi(keys).reshape(n, ci, -1)          # [n, ci, Nk]
        g = self.conv_g(keys).reshape(n, ci, -1)
        affinity = torch.einsum("nct,ncp->ntp", theta, phi)   # [n, Nq, Nk]
        if self.instantiation == "softmax":
            affinity = torch.softmax(affinity * ci ** -0.5, dim=2)
        else:
            affinity = affinity / affinity.shape[2]
        y = torch.einsum("ntg,ncg->nct", affinity, g).reshape(n, ci, t, h, w)
        y = self.conv_out(y)
        if self.norm is not None:
            y = self.norm(y)
        return x + y


def create_nonlocal(*, dim_in, dim_inner, pool_size=(1, 1, 1), instantiation="softmax", norm=nn.BatchNorm3d,
                    norm_eps=1e-5, norm_momentum=0.1):
    """Non-local block on `dim_in` channels with `dim_inner` channels inside; `pool_size` > 1 max-pools the key /
    value side (kernel = stride); `norm` follows conv_out (None: no norm)."""
    pool_size = (1, 1, 1) if pool_size is None else tuple(pool_size)
    norm_model = None if norm is None else norm(num_features=dim_in, eps=norm_eps, momentum=norm_momentum)
    pool_model = None
    if any(s > 1 for s in pool_size):
        pool_model = nn.MaxPool3d(kernel_size=pool_size, stride=pool_size, padding=[0, 0, 0])

    def pointwise(cin, cout):
        return nn.Conv3d(cin, cout, kernel_size=1, stride=1, padding=0)

    # (theta, phi, g, out are created in this order: seeded initialisation matches the reference's)
    return NonLocal(conv_theta=pointwise(dim_in, dim_inner), conv_phi=pointwise(dim_in, dim_inner),
                    conv_g=pointwise(dim_in, dim_inner), conv_out=pointwise(dim_inner, dim_in),
                    pool=pool_model, norm=norm_model, instantiation=instantiation)
