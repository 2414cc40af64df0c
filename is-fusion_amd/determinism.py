"""Deterministic mode: bit-identical training steps run to run.

A plain per-process flag in the style of ``spconv.TRAINING_KERNELS``.  With the flag set, the four places where the library
accumulates floats with atomics (DynamicScatter sum / mean, Point-to-Grid backward, both MSDA backwards) run their
``isf_*_det`` entries, which accumulate exactly in 64-bit fixed point and so do not depend on the order the contributions
arrive in (include/isf_hip.h, DETERMINISTIC ENTRIES).  The default entries, kernels and Python paths are untouched with
the flag off.  Two more things tools/step_digest.py found in the backward pass ride on the same flag:
  * the gathers of the mined instance cells and of the head's proposal cells (fusion_ops.gather_cells) take their
    backward from isf_gather_cells_backward instead of autograd's scatter_add (fp32 atomics; a cell can be named twice);
  * the stock convolutions (MIOpen) are asked for deterministic algorithms: torch.backends.cudnn.deterministic is set to
    True while the mode is on and put back to what it was when the mode goes off.

An autograd Function reads the flag in ``forward`` and keeps it on ``ctx`` for its ``backward``: a backward that runs
outside the ``with`` block still matches its forward.

This module imports nothing of the package, no tensor library and no kernel library: the three calls work without a GPU.
"""
import contextlib
import sys

_ENABLED = False
_MIOPEN_BEFORE = None        # torch.backends.cudnn.deterministic as the mode found it (None: the mode is off / never set it)


def _stock_convs(flag):
    """MIOpen's deterministic attribute follows the mode.  Only when the tensor library is loaded already (nothing of it
    can have run otherwise, and importing isfusion_amd loads it)."""
    global _MIOPEN_BEFORE
    torch = sys.modules.get("torch")
    if torch is None:
        return
    if flag and _MIOPEN_BEFORE is None:
        _MIOPEN_BEFORE = bool(torch.backends.cudnn.deterministic)
        torch.backends.cudnn.deterministic = True
    elif not flag and _MIOPEN_BEFORE is not None:
        torch.backends.cudnn.deterministic = _MIOPEN_BEFORE
        _MIOPEN_BEFORE = None


def set_deterministic(flag):
    """Switch the mode on or off for this process."""
    global _ENABLED
    _ENABLED = bool(flag)
    _stock_convs(_ENABLED)


def is_deterministic():
    return _ENABLED


@contextlib.contextmanager
def deterministic(flag=True):
    """``with deterministic():`` -- the mode inside the block, the previous state after it (also on an exception); nests."""
    previous = _ENABLED
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(previous)


def entry(name):
    """The C entry a call site runs: ``name`` by default, ``name + "_det"`` under the mode."""
    return name + "_det" if _ENABLED else name
