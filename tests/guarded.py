"""Guarded, pre-filled device buffers for tests/test_gpu_buffers.py (a plain module, no fixtures).

Every caller-owned device buffer of the package comes from two helpers, ``ops._scratch`` (byte buffers sized by a ``csd_*_bytes`` entry:
scratch, workspaces, packed weights) and ``ops._out`` (result tensors).  ``seam(fill)`` replaces both for the length of a ``with`` block:
each buffer then lies between two 1 MiB guards, guards and body are filled with one byte, and the block's record keeps a checker per
buffer.  Fill 0x00 is the benign baseline; with fill 0xFF every fp32, fp16, fp64 and e4m3 lane of a buffer is a NaN, so a kernel that
reads a byte the library did not write first turns its output into NaN (or into different bits), and a kernel that writes outside the
declared size changes a guard byte.

The record also notes which sizing entry declared the size of each byte buffer: the ``csd_*_bytes`` functions of the loaded library
are wrapped while the block is open, and a request of ``n`` bytes is attributed to the latest sizing call that returned ``n``.

``SIZING`` maps every sizing entry of the ABI to the tests of test_gpu_buffers.py that run under a buffer sized by it;
tests/test_host_logic.py checks on the CPU that the table is complete, and the GPU tests assert from the record that the entries of
their rows really sized a buffer of the run.
"""
import contextlib

import torch

GUARD = 1 << 20          # bytes on either side of a body; a multiple of 4096, so the body keeps the allocator's alignment

_NETWORKS = ['test_network_forward', 'test_ncsnpp_forward', 'test_nf96_network_forward', 'test_nf128_network_forward',
             'test_elu_network_forward', 'test_network_forward_two_batch_chunks', 'test_pc_sampling', 'test_pc_inpainting',
             'test_pc_step_forms']
# sizing entry -> tests of tests/test_gpu_buffers.py that run in a buffer of exactly the size the entry declared: a function name
# (every parametrisation) or one test id with its parameters
SIZING = {
    'csd_unet_packed_bytes': _NETWORKS,
    'csd_unet_workspace_bytes': _NETWORKS,
    'csd_pc_scratch_bytes': ['test_pc_sampling', 'test_pc_step_forms'],
    'csd_pc_inpaint_scratch_bytes': ['test_pc_inpainting'],
    'csd_unet_train_workspace_bytes': ['test_planned_training', 'test_eval_input_gradient', 'test_likelihood'],
    'csd_update_scratch_bytes': ['test_langevin_step'],
    'csd_groupnorm_scratch_bytes': ['test_groupnorm_act', 'test_groupnorm_act_backward[nchw]'],
    'csd_conv_scratch_bytes': ['test_conv2d', 'test_conv2d_nhwc', 'test_conv_backward'],
    'csd_attention_scratch_bytes': ['test_attention', 'test_attention_backward_nchw'],
    'csd_fir_pyr_conv_scratch_bytes': ['test_fir_pyr_conv'],
    'csd_conv_wgrad_scratch_bytes': ['test_conv_backward', 'test_conv2d_nhwc'],
    'csd_attention_backward_scratch_bytes': ['test_attention_backward_packed', 'test_attention_backward_nchw'],
    'csd_conv3x3_block_scratch_bytes': ['test_conv3x3_block'],
    'csd_groupnorm_nhwc_scratch_bytes': ['test_groupnorm_act_backward[nhwc]', 'test_ddpm3d_training'],
    'csd_sum_pixels_scratch_bytes': ['test_sum_pixels_nhwc'],
    'csd_global_norm_scratch_bytes': ['test_global_norm'],
    'csd_pf_ode_scratch_bytes': ['test_likelihood'],
    'csd_ode_scratch_bytes': ['test_device_rk45'],
    'csd_conv3d_block_scratch_bytes': ['test_conv3d_block', 'test_conv3d_gradients', 'test_ddpm3d_forward', 'test_ddpm3d_training'],
    'csd_conv3d_wgrad_scratch_bytes': ['test_conv3d_gradients', 'test_ddpm3d_training'],
    'csd_conv3d_dgrad_scale_scratch_bytes': ['test_conv3d_gradients', 'test_ddpm3d_training'],
    'csd_groupnorm_scale_shift_scratch_bytes': ['test_groupnorm_scale_shift', 'test_ddpm3d_forward'],
}


def entries_of(function, test_id=None):
    """the sizing entries whose row names the test function or this one test id"""
    return sorted(e for e, tests in SIZING.items() if function in tests or (test_id is not None and test_id in tests))


def guarded(nbytes, device, fill):
    """(body, check): ``body`` is a uint8 view of exactly ``nbytes`` bytes with ``GUARD`` bytes before and behind it, everything
    filled with the byte ``fill``; ``check()`` asserts that both guards still hold it."""
    nbytes = int(nbytes)
    raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=device)
    body = raw[GUARD:GUARD + nbytes]
    assert (nbytes == 0 or body.data_ptr() == raw.data_ptr() + GUARD) and body.numel() == nbytes and body.is_contiguous()

    def check(what=''):
        lo = int((raw[:GUARD] != fill).sum())
        hi = int((raw[GUARD + nbytes:] != fill).sum())
        assert lo == 0 and hi == 0, '%s (%d bytes): %d guard bytes changed in front of the buffer, %d behind it' % (what, nbytes, lo, hi)

    return body, check


class Record:
    """what one ``seam`` block handed out"""

    def __init__(self, fill):
        self.fill = fill
        self.checks = []          # (description, checker) per buffer
        self.sized_by = {}        # sizing entry (None: no sizing call returned the requested size) -> number of buffers
        self.sizing_calls = []    # (entry, result) in call order
        self.outputs = 0

    def check_guards(self):
        for what, chk in self.checks:
            chk(what)

    def assert_sized_by(self, entries):
        assert None not in self.sized_by, 'a byte buffer of a size that no csd_*_bytes call declared: %r' % (self.sized_by,)
        for e in entries:
            assert self.sized_by.get(e, 0) > 0, '%s sized no buffer of this run (%r)' % (e, self.sized_by)


@contextlib.contextmanager
def seam(fill):
    """hand out guarded buffers filled with ``fill`` from ops._scratch / ops._out; yields the Record"""
    from conditional_score_diffusion_amd import _lib, ops
    rec = Record(fill)
    l = _lib.lib()
    real = {name: getattr(l, name) for name in SIZING}

    def wrap(name, fn):
        def sizing(*args):
            n = fn(*args)
            rec.sizing_calls.append((name, int(n)))
            return n
        return sizing

    def scratch(nbytes, device):
        nbytes = int(nbytes)
        entry = next((name for name, n in reversed(rec.sizing_calls) if n == nbytes), None)
        rec.sized_by[entry] = rec.sized_by.get(entry, 0) + 1
        body, chk = guarded(nbytes or 256, device, fill)
        rec.checks.append(('bytes sized by %s' % entry, chk))
        return body

    def out(shape, dtype, device):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for s in shape:
            n *= int(s)
        body, chk = guarded(n * torch.empty(0, dtype=dtype).element_size(), device, fill)
        rec.checks.append(('output %s %s' % (shape, dtype), chk))
        rec.outputs += 1
        return body.view(dtype).view(shape)

    saved = (ops._scratch, ops._out)
    for name, fn in real.items():
        setattr(l, name, wrap(name, fn))
    ops._scratch, ops._out = scratch, out
    try:
        yield rec
    finally:
        ops._scratch, ops._out = saved
        for name, fn in real.items():
            setattr(l, name, fn)


def reset_model_buffers(model):
    """drop the buffers a network caches on the instance (packed weights, activation and training workspace): the next call
    allocates them through the seam and packs again"""
    for attr in ('_packed', '_packed_key', '_ws', '_train_ws'):
        if hasattr(model, attr):
            setattr(model, attr, None)
