"""Record the REAL reference's non-local block (imported through oracle/ref_shim.py) -> tests/golden/nonlocal_small.pt:
three configurations on dim_in 16, dim_inner 8, input [2, 16, 2, 4, 4].  Runs only where the reference exists; the
fixture is committed.

    python tests/golden/make_nonlocal_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim  # noqa: E402

SEED = 1234
SHAPE = (2, 16, 2, 4, 4)
CASES = {
    "softmax": dict(dim_in=16, dim_inner=8, pool_size=(1, 1, 1), instantiation="softmax"),
    "softmax_pool": dict(dim_in=16, dim_inner=8, pool_size=(1, 2, 2), instantiation="softmax"),
    "dot_product_pool": dict(dim_in=16, dim_inner=8, pool_size=(1, 2, 2), instantiation="dot_product", norm=None),
}


def calibrate(m, seed):
    """BatchNorm away from its initial state (gamma, beta and the running statistics), from the seed: at gamma = 0 the
    block is the identity, at the initial statistics the norm is nearly one."""
    g = torch.Generator().manual_seed(seed)
    if m.norm is not None:
        with torch.no_grad():
            m.norm.weight.copy_(torch.rand(m.norm.weight.shape, generator=g) + 0.5)
            m.norm.bias.copy_(torch.randn(m.norm.bias.shape, generator=g) * 0.2)
        m.train()
        with torch.no_grad():
            for _ in range(3):
                m(torch.randn(SHAPE, generator=g) * 2.0 + 0.3)
    return m.eval()


def main():
    ref_shim.install()
    from pytorchvideo.layers.nonlocal_net import create_nonlocal
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(SEED))
    out = {"seed": SEED, "input": x, "cases": {}}
    for i, (name, kwargs) in enumerate(CASES.items()):
        torch.manual_seed(SEED + i)
        m = calibrate(create_nonlocal(**kwargs), SEED + 100 + i)
        with torch.no_grad():
            y = m(x)
        assert (y - x).abs().max() > 1e-2, "the block must not be the identity"
        out["cases"][name] = {"kwargs": kwargs, "seed": SEED + i, "output": y,
                              "state_dict": {k: v.clone() for k, v in m.state_dict().items()}}
    path = os.path.join(HERE, "nonlocal_small.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
