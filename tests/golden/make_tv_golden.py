#!/usr/bin/env python3
"""Generate tests/golden/tv.npz by IMPORTING THE REFERENCE's modules/utils.py and calling its own total_variation_loss
(lines 360-369) on a random image, with the gradient its own autograd gives.  Only data travels: the image, the value
and image.grad.  A handful of neighbouring pixels are set equal, so that the derivative of abs at 0 occurs.  The
reference's utils imports plotting and image libraries at module scope for other helpers; empty stubs stand in for
whichever of them is absent, as make_golden.py does.

    python3 tests/golden/make_tv_golden.py /path/to/reference
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (1, 3, 37, 29)
# (channel, row, column, direction): the pixel and its lower (0) or right (1) neighbour are made equal
TIES = [(0, 0, 0, 0), (0, 0, 0, 1), (1, 5, 7, 1), (1, 5, 8, 1), (2, 35, 28, 0), (2, 36, 26, 1), (0, 18, 14, 0),
        (1, 18, 14, 0), (2, 18, 14, 1)]


class _Stub(types.ModuleType):
    """A module whose every attribute is another stub (``import a.b as c`` and ``from a import b`` both work)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _Stub(self.__name__ + "." + name)
        sys.modules[sub.__name__] = sub
        setattr(self, name, sub)
        return sub


class _StubFinder:
    """Stands in for a top-level package that is not installed, and for its submodules."""

    def __init__(self):
        self.roots = set()

    def find_spec(self, name, path=None, target=None):
        import importlib.machinery
        if name.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def import_reference_utils(ref):
    finder = _StubFinder()
    sys.meta_path.append(finder)
    sys.path.insert(0, ref)
    for _ in range(32):                       # every absent third-party import becomes a stub, one per attempt
        try:
            return importlib.import_module("modules.utils")
        except ImportError as e:
            if not e.name or e.name.split(".")[0] in finder.roots or e.name.startswith("modules"):
                raise
            finder.roots.add(e.name.split(".")[0])
            for k in [k for k in sys.modules if k == "modules" or k.startswith("modules.")]:
                del sys.modules[k]
    raise RuntimeError("could not import the reference's modules.utils")


def main():
    utils = import_reference_utils(sys.argv[1])
    image = np.random.default_rng(7).standard_normal(SHAPE).astype(np.float32)
    for c, i, j, right in TIES:
        image[0, c, i + (1 - right), j + right] = image[0, c, i, j]
    x = torch.tensor(image, requires_grad=True)
    tv = utils.total_variation_loss(x)
    tv.backward()
    assert tv.dtype == torch.float32 and x.grad.shape == x.shape
    out = os.path.join(HERE, "tv.npz")
    np.savez(out, image=image, tv=tv.detach().numpy(), grad=x.grad.numpy(), ties=np.array(TIES, np.int64))
    print(out, "image", image.shape, "tv", float(tv.detach()), "grad values", np.unique(x.grad.numpy()))


if __name__ == "__main__":
    main()
