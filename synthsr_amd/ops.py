"""Thin tensor-level wrappers over the C ABI (include/synthsr_hip.h) for the U-Net kernels.

Tensors are contiguous float32 device tensors in NDHWC order ([d0,d1,d2,C]; batch handled by the
caller).  No autograd, no CPU fallback: each function is one (or a few) kernel launches on the
current stream.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

BN_EPS = 1e-3  # keras.layers.BatchNormalization default epsilon (Keras 2.3.1)

# optional per-launch timing of the conv kernels (bench.py): list of (kind, shape, Cin, Cout, start_evt, end_evt)
_prof = None


# The context handed to every fp32 conv entry point (include/synthsr_hip.h: synthsr_conv_ctx).  The LIBRARY holds no arithmetic
# state and owns no scratch: this module keeps the default arithmetic for the host code that does not pass its own (unet.py,
# critic.py, the tests), one context PER (device, stream) -- each with its own torch-allocated workspace, so that two streams of
# one device never share scratch -- and a counter that moves when the arithmetic is replaced: packed weights are only valid under
# the arithmetic they were packed with (check_layout_epoch).
_arith = 1
_ctx_epoch = 0
_ctx_host = _lib.ConvCtx(arithmetic=1)        # host-only queries (plans, packed sizes): no workspace, usable without a GPU
_ctxs = {}                                    # (device, stream handle) -> (ConvCtx, its workspace tensor)
_ctx_last = (None, None)


def conv_ctx_host():
    """ctypes reference to a workspace-less context of the current arithmetic (host-only entry points)"""
    return ctypes.byref(_ctx_host)


def conv_ctx():
    """ctypes reference to the conv context of the CURRENT device and stream (created on first use: the current arithmetic and
    a workspace of synthsr_conv_workspace_bytes() that torch allocates)"""
    global _ctx_last
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    if _ctx_last[0] == key:
        return _ctx_last[1]
    e = _ctxs.get(key)
    if e is None:
        n = int(_L().synthsr_conv_workspace_bytes())
        ws = torch.empty(n, dtype=torch.uint8, device='cuda:%d' % key[0])
        e = (_lib.ConvCtx(arithmetic=_arith, workspace=ws.data_ptr(), workspace_bytes=n), ws)
        _ctxs[key] = e
    _ctx_last = (key, ctypes.byref(e[0]))
    return _ctx_last[1]


def set_conv_arithmetic(name):
    """replaces this module's default conv arithmetic: 'split' (default) = fp32 convolutions on the bf16 matrix cores through three
    bf16 pieces per operand and six exact partial products (fp32 accumulation, as accurate as the fp32 matrix instructions:
    tests/test_split_gpu.py); 'split9' = the same with all nine partial products (every fp32 product reproduced exactly, 1.5x
    the matrix instructions); 'fp32_mfma' = fp32 matrix instructions everywhere.  Networks must re-pack their weights
    (`repack()`) before their next forward / backward: conv_layout_epoch moves and check_layout_epoch raises on stale packed
    weights.  Returns the previous setting."""
    global _arith, _ctx_epoch, _ctx_host, _ctx_last
    if name not in _lib.CONV_ARITHMETICS:
        raise ValueError('conv arithmetic should be one of %s' % (_lib.CONV_ARITHMETICS,))
    prev = conv_arithmetic()
    if name != prev:
        _arith = _lib.CONV_ARITHMETICS.index(name)
        _ctx_host = _lib.ConvCtx(arithmetic=_arith)
        for key, (c, ws) in list(_ctxs.items()):   # fresh structs (a launch in flight has read its own already): same workspaces
            _ctxs[key] = (_lib.ConvCtx(arithmetic=_arith, workspace=ws.data_ptr(), workspace_bytes=ws.numel()), ws)
        _ctx_last = (None, None)
        _ctx_epoch += 1
    return prev


def check_layout_epoch(epoch, what):
    """a network's packed weights were laid out under conv_layout_epoch() == epoch: using them under another arithmetic would
    plan for one layout and read another (silently wrong results on the Cout = 24 layers) -- raise instead"""
    if epoch is not None and epoch != _ctx_epoch:
        raise RuntimeError('%s: the conv arithmetic changed (ops.set_conv_arithmetic) since these weights were packed; call '
                           'repack() first' % what)


def conv_arithmetic():
    return _lib.CONV_ARITHMETICS[_arith]


def conv_layout_epoch():
    """moves whenever the default conv context was replaced: packed weights of an older epoch are stale -- their size or
    fragment order may belong to another plan"""
    return _ctx_epoch


def conv_runs_split(kind, shape, cin, cout):
    """whether a conv launch of this kind ('conv3d_fwd' | 'conv3d_dgrad' | 'conv3d_wgrad' | 'conv3d_up_fwd' | 'conv3d_up_dgrad',
    the names of the profile records) runs on the split kernels under the CURRENT arithmetic (mirrors the dispatcher: csrc/conv3d.hip plan_fwd /
    dispatch_wgrad); used by the benchmarks to price a kernel against the right peak"""
    kinds = ('conv3d_fwd', 'conv3d_dgrad', 'conv3d_wgrad', 'conv3d_up_fwd', 'conv3d_up_dgrad', 'conv3d_up_wgrad')
    if conv_arithmetic() == 'fp32_mfma' or kind not in kinds:
        return False
    d0, d1, d2 = [int(v) for v in shape[:3]]
    if kind == 'conv3d_up_wgrad':   # (low-res shape, Cl, Cout): csrc/conv3d.hip up_wgrad_takes_split
        rc = int(_L().synthsr_conv3d_up_wgrad_runs_split(conv_ctx_host(), _lib.i3((d0, d1, d2)), int(cin), int(cout)))
        if rc < 0:
            _lib.check(rc, 'conv3d_up_wgrad_runs_split')
        return rc == 1
    if kind == 'conv3d_wgrad':   # the dispatcher's own condition (csrc/conv3d.hip: wgrad_takes_split)
        rc = int(_L().synthsr_conv3d_wgrad_runs_split(conv_ctx_host(), _lib.i3((d0, d1, d2)), int(cin), int(cout)))
        if rc < 0:
            _lib.check(rc, 'conv3d_wgrad_runs_split')
        return rc == 1
    # folded decoder convs are recorded with (low-res shape, Cl, Cout): forward = plan kind 2 on (Cl -> Cout), data gradient =
    # plan kind 0 on (Cout -> Cl)
    plan_kind, ce, co = {'conv3d_up_fwd': (2, cin, cout), 'conv3d_up_dgrad': (0, cout, cin)}.get(kind, (1, cin, cout))
    out = (ctypes.c_int64 * 8)()
    _lib.check(_L().synthsr_conv3d_plan(conv_ctx_host(), _lib.i3((d0, d1, d2)), int(ce), int(co), plan_kind, out), 'conv3d_plan')
    return int(out[2]) <= -100


def set_deterministic(on=True):
    """process-wide switch (include/synthsr_hip_tuning.h: synthsr_set_deterministic): bit-identical results run after run on
    the same inputs -- every cross-workgroup float accumulation happens in a fixed order, no split-K forward.  Scope: the
    whole PROCESS on the CURRENT device (every network, critic and predictor is switched together) and ONE stream (kernels
    of two streams must not overlap while it is on).  Returns the previous setting."""
    global _deterministic
    prev = _deterministic
    torch.cuda.synchronize()
    _lib.check(_L().synthsr_set_deterministic(int(bool(on))), 'set_deterministic')
    _deterministic = bool(on)
    if on:
        _register_det_planes(64 << 20)
    return prev


_det_planes = {}    # device -> the torch buffer registered as the private dW planes of the deterministic weight-gradient flush


def _register_det_planes(min_bytes):
    """the planes are CALLER memory (include/synthsr_hip_tuning.h: synthsr_set_deterministic_workspace): torch allocates, grown to
    1.25x the library's recorded demand whenever a weight gradient reported SYNTHSR_EWORKSPACE.  Returns whether the
    registration was short of that demand, i.e. whether a SYNTHSR_EWORKSPACE just reported was about the planes"""
    dev = torch.cuda.current_device()
    demand = int(_L().synthsr_deterministic_workspace_demand())
    want = max(int(min_bytes), int(1.25 * demand))
    cur = _det_planes.get(dev)
    have = 0 if cur is None else cur.numel()
    if have < want:
        _resize_det_planes(want)
    return have < demand


def _resize_det_planes(nbytes):
    """registers a fresh plane buffer of exactly `nbytes` on the current device (0: none) -- growth, and the tests that
    shrink or withdraw the registration.  The library never holds a pointer torch may hand to another tensor: the old
    registration is WITHDRAWN before the old buffer is released (released first: the two need not fit side by side), so an
    allocation that raises leaves no planes registered and none recorded here, and the next weight gradient reports
    SYNTHSR_EWORKSPACE and registers again (_check_wgrad; tests/test_wgrad_scratch_gpu.py:
    test_failed_plane_allocation_leaves_no_stale_registration)"""
    dev = torch.cuda.current_device()
    _lib.check(_L().synthsr_set_deterministic_workspace(None, 0), 'set_deterministic_workspace')   # synchronises the device
    _det_planes.pop(dev, None)
    if nbytes:
        new = torch.empty(int(nbytes), dtype=torch.uint8, device='cuda:%d' % dev)
        _lib.check(_L().synthsr_set_deterministic_workspace(_lib.ptr(new), new.numel()), 'set_deterministic_workspace')
        _det_planes[dev] = new


def _check_wgrad(call, what):
    """weight-gradient launches: in deterministic mode the call may report that the registered plane buffer is too small
    (nothing was launched: tests/test_wgrad_scratch_gpu.py) -- register a larger one and repeat ONCE"""
    rc = call()
    short = False
    if rc == -3 and _deterministic:
        short = _register_det_planes(0)
        rc = call()
    _lib.check(rc, what, planes=short)


def deterministic_status():
    """0 off; 1 on and every ordered flush completed in order; 2 on but a wait timed out (order not guaranteed)"""
    torch.cuda.synchronize()
    return int(_L().synthsr_deterministic_status())


_deterministic = False


def profile_start():
    global _prof
    _prof = []


def profile_stop():
    global _prof, _prof_paused
    p = _prof if _prof is not None else _prof_paused
    _prof, _prof_paused = None, None
    return p


_prof_paused = None


def profile_pause():
    """stop recording events (they cost ~8 us per launch) but keep what was collected for profile_stop()"""
    global _prof, _prof_paused
    if _prof is not None:
        _prof_paused, _prof = _prof, None


# ---- roctx ranges (tracing): named CPU-side ranges around the phases of a step and around every conv /
# generator launch, visible in `rocprofv3 --marker-trace`.  Off unless SYNTHSR_ROCTX=1 (one ctypes call per range otherwise).
_roctx = None


def _roctx_lib():
    global _roctx
    if _roctx is None:
        _roctx = False
        if os.environ.get('SYNTHSR_ROCTX') == '1':
            import ctypes
            for name in ('libroctx64.so', 'librocprofiler-sdk-roctx.so'):
                try:
                    lib = ctypes.CDLL(name)
                    lib.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    lib.roctxRangePushA.restype = ctypes.c_int
                    lib.roctxRangePop.restype = ctypes.c_int
                    _roctx = lib
                    break
                except (OSError, AttributeError):
                    continue
    return _roctx


class trace_range:
    """`with ops.trace_range('backward'):` -- a roctx range when SYNTHSR_ROCTX=1 and the marker library is present, else nothing"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        lib = _roctx_lib()
        self.on = bool(lib)
        if self.on:
            lib.roctxRangePushA(str(self.name).encode())
        return self

    def __exit__(self, *a):
        if self.on:
            _roctx.roctxRangePop()


def timed(kind, shape=(0, 0, 0), cin=0, cout=0):
    """context manager: HIP events around a region on the launch stream, recorded while profile_start() is active
    (bench.py: conv launches and the generator's kernels); free otherwise"""
    return _Timed(kind, shape, cin, cout)


class _Timed:
    def __init__(self, kind, shape, cin, cout):
        self.meta = (kind, tuple(int(s) for s in shape), int(cin), int(cout))

    def __enter__(self):
        self.rng = None
        if _roctx_lib():
            k, sh, ci, co = self.meta
            self.rng = trace_range('%s %dx%dx%d %d->%d' % (k, sh[0], sh[1], sh[2], ci, co)).__enter__()
        if _prof is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if _prof is not None:
            self.e.record()
            _prof.append(self.meta + (self.s, self.e))
        if self.rng is not None:
            self.rng.__exit__()


def _L():
    return _lib.load()


def _sym(name, t):
    """entry point `name` for float32 tensors, `name_bf16` for bfloat16 ones (same arguments)"""
    return getattr(_L(), name + '_bf16' if t.dtype == torch.bfloat16 else name)


def pack_conv_weights(w, shape, mode=0, out=None):
    """w: Keras Conv3D kernel [3,3,3,Cin,Cout] -> MFMA fragment order for a layer of spatial size `shape`
    (mode 0 fwd, 1 data-gradient)"""
    lib = _L()
    Cin, Cout = int(w.shape[3]), int(w.shape[4])
    s3 = _lib.i3(shape[:3])
    n = lib.synthsr_conv3d_pack(conv_ctx_host(), None, None, s3, Cin, Cout, mode, None)
    if n < 0:
        _lib.check(int(n), 'conv3d_pack(size)')
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.numel() == n
    r = lib.synthsr_conv3d_pack(conv_ctx(), _lib.ptr(w), _lib.ptr(out), s3, Cin, Cout, mode, _lib.stream())
    if r < 0:
        _lib.check(int(r), 'conv3d_pack')
    return out


def pack_conv_weights_ex(w, shape, ci_off, cin, mode=0, up=False, out=None):
    """pack the input-channel range [ci_off, ci_off+cin) of a Keras kernel w [3,3,3,Cin_total,Cout]; `up`: the 8 parity
    weight sets of the nearest-upsample folding (shape = LOW-RES spatial shape); up = 2: those of a stride-2 conv"""
    lib = _L()
    cin_total, cout = int(w.shape[3]), int(w.shape[4])
    s3 = _lib.i3(shape[:3])
    n = lib.synthsr_conv3d_pack_ex(conv_ctx_host(), None, None, s3, cin_total, int(ci_off), int(cin), cout, mode, int(up), None)
    if n < 0:
        _lib.check(int(n), 'conv3d_pack_ex(size)')
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.numel() == n
    r = lib.synthsr_conv3d_pack_ex(conv_ctx(), _lib.ptr(w), _lib.ptr(out), s3, cin_total, int(ci_off), int(cin), cout, mode,
                                   int(up), _lib.stream())
    if r < 0:
        _lib.check(int(r), 'conv3d_pack_ex')
    return out


def conv3d_up(lo, wpacked8, bias, addend, Cout, act=1, out=None):
    """act(conv3(UpSampling3D(2)(lo)) + addend + bias) evaluated on the low-res tensor (8 parity convs); bf16: the raw
    partial sums only (bias / addend / activation come with the skip-channel conv, conv3d_add)"""
    lib = _L()
    s = lo.shape
    if lo.dtype == torch.bfloat16:
        assert bias is None and addend is None and act == 0
        if out is None:
            out = torch.empty((2 * s[0], 2 * s[1], 2 * s[2], Cout), dtype=torch.bfloat16, device=lo.device)
        with _Timed('conv3d_bf16_up_fwd', s[:3], s[3], Cout):
            _lib.check(lib.synthsr_conv3d_bf16_up_fwd(_lib.ptr(lo), _lib.ptr(wpacked8), _lib.ptr(out), _lib.i3(s[:3]),
                                                      int(s[3]), int(Cout), _lib.stream()), 'conv3d_bf16_up_fwd')
        return out
    if out is None:
        out = torch.empty((2 * s[0], 2 * s[1], 2 * s[2], Cout), dtype=torch.float32, device=lo.device)
    with _Timed('conv3d_up_fwd', s[:3], s[3], Cout):
        _lib.check(lib.synthsr_conv3d_up_fwd(conv_ctx(), _lib.ptr(lo), _lib.ptr(wpacked8), _lib.ptr(bias), _lib.ptr(addend),
                                             _lib.ptr(out), _lib.i3(s[:3]), int(s[3]), int(Cout), int(act),
                                             _lib.stream()), 'conv3d_up_fwd')
    return out


def conv3d_up_dgrad(dout, wpacked8, Cl, out=None):
    """gradient w.r.t. the low-res tensor of conv3d_up; dout [2*lo_shape, Cout]"""
    lib = _L()
    s = dout.shape
    lo_shape = (s[0] // 2, s[1] // 2, s[2] // 2)
    if dout.dtype == torch.bfloat16:
        if out is None:
            out = torch.empty(lo_shape + (Cl,), dtype=torch.bfloat16, device=dout.device)
        scratch = _bf16_scratch.get(dout.device)   # fp32 partial planes of the split-K path (small levels)
        need = 8 * lo_shape[0] * lo_shape[1] * lo_shape[2] * int(Cl) if lo_shape[0] * lo_shape[1] * lo_shape[2] <= 32 ** 3 else 0
        if scratch is None or scratch.numel() < need:
            scratch = _bf16_scratch[dout.device] = torch.empty(max(need, 1 << 20), dtype=torch.float32, device=dout.device)
        with _Timed('conv3d_bf16_up_dgrad', lo_shape, Cl, s[3]):
            _lib.check(lib.synthsr_conv3d_bf16_up_dgrad(_lib.ptr(dout), _lib.ptr(wpacked8), _lib.ptr(out), _lib.i3(lo_shape),
                                                        int(Cl), int(s[3]), _lib.ptr(scratch), scratch.numel(),
                                                        _lib.stream()), 'conv3d_bf16_up_dgrad')
        return out
    if out is None:
        out = torch.empty(lo_shape + (Cl,), dtype=torch.float32, device=dout.device)
    with _Timed('conv3d_up_dgrad', lo_shape, Cl, s[3]):
        _lib.check(lib.synthsr_conv3d_up_dgrad(conv_ctx(), _lib.ptr(dout), _lib.ptr(wpacked8), _lib.ptr(out), _lib.i3(lo_shape),
                                               int(Cl), int(s[3]), _lib.stream()), 'conv3d_up_dgrad')
    return out


def conv3d_up_wgrad(lo, dout, dwc, dw, ci_off, dwc_is_zero=False):
    """weight gradient of the up-sampled channel range: dwc [8,27,Cl,Cout] scratch, dw (+=).  dwc is zeroed here unless the
    caller vouches that it is all zeros (`dwc_is_zero`): the unpack kernel CONSUMES the partials and leaves zeros behind, so a
    persistent scratch buffer needs the memset once, not once per call (UNet3D keeps that book; every kernel variant:
    tests/test_wgrad_scratch_gpu.py: test_dwc_is_all_zeros_after_unpack_and_reusable)"""
    lib = _L()
    s = lo.shape
    if not dwc_is_zero:
        dwc.zero_()
    if lo.dtype == torch.bfloat16:
        with _Timed('conv3d_bf16_up_wgrad', s[:3], s[3], dout.shape[3]):
            _check_wgrad(lambda: lib.synthsr_conv3d_bf16_up_wgrad(_lib.ptr(lo), _lib.ptr(dout), _lib.ptr(dwc), _lib.i3(s[:3]), int(s[3]),
                                                        int(dout.shape[3]), _lib.stream()), 'conv3d_bf16_up_wgrad')
        _lib.check(lib.synthsr_conv3d_up_unpack(_lib.ptr(dwc), _lib.ptr(dw), int(dw.shape[3]), int(ci_off), int(s[3]),
                                                int(dout.shape[3]), _lib.stream()), 'conv3d_up_unpack')
        return dw
    with _Timed('conv3d_up_wgrad', s[:3], s[3], dout.shape[3]):
        _check_wgrad(lambda: lib.synthsr_conv3d_up_wgrad(conv_ctx(), _lib.ptr(lo), _lib.ptr(dout), _lib.ptr(dwc), _lib.i3(s[:3]),
                                               int(s[3]), int(dout.shape[3]), _lib.stream()), 'conv3d_up_wgrad')
    _lib.check(lib.synthsr_conv3d_up_unpack(_lib.ptr(dwc), _lib.ptr(dw), int(dw.shape[3]), int(ci_off), int(s[3]),
                                            int(dout.shape[3]), _lib.stream()), 'conv3d_up_unpack')
    return dw


def conv3d_wgrad_part(x, dout, dw, ci_off, dbias=None):
    """dw [3,3,3,Cin_total,Cout] += gradient of the input-channel range [ci_off, ci_off + x.shape[3]);
    dbias [Cout] (optional) += sum over voxels of dout"""
    lib = _L()
    s = x.shape
    if x.dtype == torch.bfloat16:
        with _Timed('conv3d_bf16_wgrad', s[:3], s[3], dout.shape[3]):
            _check_wgrad(lambda: lib.synthsr_conv3d_bf16_wgrad_part(_lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(dbias),
                                                          _lib.i3(s[:3]), int(dw.shape[3]), int(ci_off), int(s[3]),
                                                          int(dout.shape[3]), _lib.stream()), 'conv3d_bf16_wgrad_part')
        return dw
    with _Timed('conv3d_wgrad', s[:3], s[3], dout.shape[3]):
        _check_wgrad(lambda: lib.synthsr_conv3d_wgrad_bias(conv_ctx(), _lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(dbias),
                                                 _lib.i3(s[:3]), int(dw.shape[3]), int(ci_off), int(s[3]),
                                                 int(dout.shape[3]), _lib.stream()), 'conv3d_wgrad_bias')
    return dw


def conv3d(x, wpacked, bias, Cout, act=1, out=None):
    """x [d0,d1,d2,Cin] -> [d0,d1,d2,Cout]; act: 0 linear, 1 ELU, 3 ReLU (bf16: the same codes, ReLU = act 3 at alpha 0)"""
    if x.dtype == torch.bfloat16:
        return conv3d_bf16(x, wpacked, bias, Cout, act, out=out)
    lib = _L()
    s = x.shape
    if out is None:
        out = torch.empty((s[0], s[1], s[2], Cout), dtype=torch.float32, device=x.device)
    with _Timed('conv3d_fwd' if bias is not None else 'conv3d_dgrad', s[:3], s[3], Cout):
        _lib.check(lib.synthsr_conv3d_fwd(conv_ctx(), _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out),
                                          _lib.i3(s[:3]), int(s[3]), int(Cout), int(act), _lib.stream()), 'conv3d_fwd')
    return out


def conv3d_stats(x, wpacked, bias, Cout, stats, ws, act=1, out=None):
    """conv3d + BatchNorm batch statistics of its output (fused into the conv epilogue where the kernel supports it)"""
    if x.dtype == torch.bfloat16:
        return conv3d_bf16(x, wpacked, bias, Cout, act, stats=stats, out=out)
    lib = _L()
    s = x.shape
    if out is None:
        out = torch.empty((s[0], s[1], s[2], Cout), dtype=torch.float32, device=x.device)
    with _Timed('conv3d_fwd', s[:3], s[3], Cout):
        _lib.check(lib.synthsr_conv3d_fwd_stats(conv_ctx(), _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out),
                                                _lib.i3(s[:3]), int(s[3]), int(Cout), int(act), _lib.ptr(stats),
                                                _lib.ptr(ws), _lib.stream()), 'conv3d_fwd_stats')
    return out


def conv3d_add(x, wpacked, bias, addend, Cout, act=1, out=None):
    """act 0/1/3: act(conv3(x) + addend + bias), `addend` may be `out` itself (in-place accumulation);
    act 2 / 4: conv3(x) * elu'(addend) / relu'(addend) -- data gradient fused with the ELU / ReLU backward of the layer that
    produced `addend`"""
    if x.dtype == torch.bfloat16:
        if act == 0:
            raise NotImplementedError('bf16: addend epilogues are act(conv + bias + addend) (act 1 / 3) and conv * act\'(addend) '
                                      '(act 2 / 4)')
        return conv3d_bf16(x, wpacked, bias, Cout, {1: 5, 2: 2, 3: 6, 4: 4}[act], below=addend, out=out)
    lib = _L()
    s = x.shape
    if out is None:
        out = torch.empty((s[0], s[1], s[2], Cout), dtype=torch.float32, device=x.device)
    with _Timed('conv3d_dgrad' if act in (2, 4) else 'conv3d_fwd', s[:3], s[3], Cout):
        _lib.check(lib.synthsr_conv3d_fwd_add(conv_ctx(), _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(addend),
                                              _lib.ptr(out), _lib.i3(s[:3]), int(s[3]), int(Cout), int(act),
                                              _lib.stream()), 'conv3d_fwd_add')
    return out


def conv3d_wgrad(x, dout, dw, dbias=None):
    """dw [3,3,3,Cin,Cout] += sum_v x[v+t-1] (x) dout[v]; dbias [Cout] (optional) += sum_v dout[v]"""
    if x.dtype == torch.bfloat16:
        return conv3d_wgrad_bf16(x, dout, dw, dbias)
    return conv3d_wgrad_part(x, dout, dw, 0, dbias)


def elu_bwd(dy, y, dy2=None, dbias=None, out=None, act=1):
    """dz = (dy + dy2) * act'(y) (act 1 ELU, 3 ReLU: y the stored activation output); dbias += sum dz"""
    C = int(y.shape[-1])
    nvox = y.numel() // C
    if out is None:
        out = torch.empty_like(y)
    _lib.check(_sym('synthsr_act_bwd', y)(_lib.ptr(dy), _lib.ptr(dy2), _lib.ptr(y), _lib.ptr(out), _lib.ptr(dbias), nvox, C,
                                          int(act), _lib.stream()), 'act_bwd')
    return out


def scale_channels(x, scale, out=None):
    """out[b, ..., c] = x[b, ..., c] * scale[b, c]: the dropped-out tensor of a batch with one feature mask per sample
    (KL.Dropout(noise_shape=[None, 1, 1, 1, C]), ext/neuron/models.py:320-324); x: the B volumes stacked along the first
    axis ([B * d0, d1, d2, C], fp32 or bf16; scale float32); in place allowed"""
    C = int(x.shape[-1])
    B = int(scale.shape[0])
    if x.dtype not in (torch.float32, torch.bfloat16) or scale.dtype != torch.float32 or tuple(scale.shape) != (B, C) or \
            (x.numel() // C) % B:
        raise ValueError('scale_channels: B volumes stacked along the first axis, and a float32 scale [B, C]')
    if out is None:
        out = torch.empty_like(x)
    nvox = x.numel() // C
    _lib.check(_sym('synthsr_scale_channels', x)(_lib.ptr(x), _lib.ptr(out), nvox, C, _lib.ptr(scale), nvox // B, _lib.stream()),
               'scale_channels')
    return out


def elu_bwd_drop(dy, y, drop, dy2=None, dbias=None, out=None, bn=None, head=None, eps=BN_EPS, act=1):
    """ELU backward of a conv output y ([B * d0, d1, d2, C]) whose consumer read drop[b, c] * y (see synthsr_elu_bwd_drop);
    bn = (stats, gamma, sums) when that consumer is a BatchNorm, head = (dpred, whead) for the rank-1 gradient of the head"""
    C = int(y.shape[-1])
    B = int(drop.shape[0])
    if out is None:
        out = torch.empty_like(y)
    stats, gamma, sums = bn if bn is not None else (None, None, None)
    dpred, whead = head if head is not None else (None, None)
    nvox = y.numel() // C
    _lib.check(_sym('synthsr_act_bwd_drop', y)(_lib.ptr(dy), _lib.ptr(dy2), _lib.ptr(y), _lib.ptr(out), _lib.ptr(dbias), nvox, C,
                                               _lib.ptr(stats), _lib.ptr(gamma), eps, _lib.ptr(sums), _lib.ptr(dpred),
                                               _lib.ptr(whead), _lib.ptr(drop), nvox // B, int(act), _lib.stream()),
               'act_bwd_drop')
    return out


def bn_reduce_bwd(dy, x, stats, sums, eps=BN_EPS):
    """pass 1 of the BN backward: sums [2C] (zeroed by caller) += [sum dy, sum dy*xhat]"""
    C = int(x.shape[-1])
    _lib.check(_sym('synthsr_bn_bwd_reduce', x)(_lib.ptr(dy), _lib.ptr(x), x.numel() // C, C, _lib.ptr(stats), eps,
                                         _lib.ptr(sums), _lib.stream()), 'bn_bwd_reduce')
    return sums


def bn_elu_bwd(dy, y, stats, gamma, sums, dy2=None, dbias=None, out=None, eps=BN_EPS, act=1):
    """fused pass 2 of the BN backward + ELU (act 1) / ReLU (act 3) backward (dy = gradient w.r.t. BN(y))"""
    C = int(y.shape[-1])
    if out is None:
        out = torch.empty_like(y)
    _lib.check(_sym('synthsr_bn_act_bwd', y)(_lib.ptr(dy), _lib.ptr(dy2), _lib.ptr(y), _lib.ptr(out), _lib.ptr(dbias),
                                             y.numel() // C, C, _lib.ptr(stats), _lib.ptr(gamma), eps, _lib.ptr(sums),
                                             int(act), _lib.stream()), 'bn_act_bwd')
    return out


def bn_pool_elu_bwd(dpool, y, stats, gamma, beta, sums, dy2=None, dbias=None, out=None, eps=BN_EPS, act=1):
    """MaxPooling3D backward + BN backward (pass 2) + ELU backward of an encoder level in one pass: dpool = gradient w.r.t.
    maxpool(BN(y)), sums from bn_maxpool_bwd(..., out=False, sums=sums); bit-identical to bn_maxpool_bwd + bn_elu_bwd"""
    s = y.shape
    if out is None:
        out = torch.empty_like(y)
    _lib.check(_sym('synthsr_bn_pool_act_bwd', y)(_lib.ptr(dpool), _lib.ptr(y), _lib.ptr(dy2), _lib.ptr(out), _lib.ptr(dbias),
                                                  _lib.i3(s[:3]), int(s[3]), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                  _lib.ptr(sums), eps, int(act), _lib.stream()), 'bn_pool_act_bwd')
    return out


def bn_stats(x, stats, ws):
    C = int(x.shape[-1])
    _lib.check(_sym('synthsr_bn_stats', x)(_lib.ptr(x), x.numel() // C, C, _lib.ptr(stats), _lib.ptr(ws), _lib.stream()),
               'bn_stats')
    return stats


def bn_apply(x, stats, gamma, beta, out=None, eps=BN_EPS):
    C = int(x.shape[-1])
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_sym('synthsr_bn_apply', x)(_lib.ptr(x), _lib.ptr(out), x.numel() // C, C, _lib.ptr(stats), _lib.ptr(gamma),
                                           _lib.ptr(beta), eps, _lib.stream()), 'bn_apply')
    return out


def bn_maxpool(x, stats, gamma, beta, out=None, eps=BN_EPS):
    s = x.shape
    if out is None:
        out = torch.empty((s[0] // 2, s[1] // 2, s[2] // 2, s[3]), dtype=x.dtype, device=x.device)
    _lib.check(_sym('synthsr_bn_maxpool', x)(_lib.ptr(x), _lib.ptr(out), _lib.i3(s[:3]), int(s[3]), _lib.ptr(stats),
                                      _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.stream()), 'bn_maxpool')
    return out


def bn_maxpool_bwd(dy, x, stats, gamma, beta, out=None, eps=BN_EPS, sums=None):
    """gradient of maxpool(BN(x)) w.r.t. BN(x); sums [2C] (optional, += ) = bn_reduce_bwd(result, x) for free;
    out=False (with sums): the sums only, the routed gradient is not written (bn_pool_elu_bwd re-derives it)"""
    s = x.shape
    if out is False:
        assert sums is not None
        out = None
    elif out is None:
        out = torch.empty_like(x)
    _lib.check(_sym('synthsr_bn_maxpool_bwd_ex', x)(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(out), _lib.i3(s[:3]), int(s[3]),
                                             _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.ptr(sums),
                                             _lib.stream()), 'bn_maxpool_bwd')
    return out


def bn_bwd(dy, x, stats, gamma, sums, out=None, eps=BN_EPS):
    """sums [2C] (zeroed by caller) receives [sum dy (=dbeta), sum dy*xhat (=dgamma)]; returns dx"""
    lib = _L()
    C = int(x.shape[-1])
    nvox = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_sym('synthsr_bn_bwd_reduce', x)(_lib.ptr(dy), _lib.ptr(x), nvox, C, _lib.ptr(stats), eps, _lib.ptr(sums),
                                         _lib.stream()), 'bn_bwd_reduce')
    _lib.check(lib.synthsr_bn_bwd_apply(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(out), nvox, C, _lib.ptr(stats),
                                        _lib.ptr(gamma), eps, _lib.ptr(sums), _lib.stream()), 'bn_bwd_apply')
    return out


def upsample_concat(skip, lo, stats, gamma, beta, out=None, eps=BN_EPS):
    s = skip.shape
    Cs, Cl = int(s[3]), int(lo.shape[3])
    if out is None:
        out = torch.empty((s[0], s[1], s[2], Cs + Cl), dtype=skip.dtype, device=skip.device)
    _lib.check(_sym('synthsr_upsample_concat', skip)(_lib.ptr(skip), _lib.ptr(lo), _lib.ptr(out), _lib.i3(s[:3]), Cs, Cl,
                                           _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.stream()),
               'upsample_concat')
    return out


def upsample_concat_bwd(dcat, Cs, Cl, dskip=None, dlo=None):
    s = dcat.shape
    if dskip is None:
        dskip = torch.empty((s[0], s[1], s[2], Cs), dtype=dcat.dtype, device=dcat.device)
    if dlo is None:
        dlo = torch.empty((s[0] // 2, s[1] // 2, s[2] // 2, Cl), dtype=dcat.dtype, device=dcat.device)
    _lib.check(_sym('synthsr_upsample_concat_bwd', dcat)(_lib.ptr(dcat), _lib.ptr(dskip), _lib.ptr(dlo), _lib.i3(s[:3]), Cs, Cl,
                                               _lib.stream()), 'upsample_concat_bwd')
    return dskip, dlo


def head_l1_fwd(x, stats, gamma, beta, w, b, target, loss, pred=None, dpred=None, residual=None, res_stride=1,
                res_off=0, eps=BN_EPS):
    lib = _L()
    C = int(x.shape[-1])
    nvox = x.numel() // C
    _lib.check(lib.synthsr_head_l1_fwd(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                       _lib.ptr(w), _lib.ptr(b), _lib.ptr(residual), int(res_stride), int(res_off),
                                       _lib.ptr(target), _lib.ptr(pred), _lib.ptr(dpred), _lib.ptr(loss),
                                       _lib.stream()), 'head_l1_fwd')
    return loss


LOSS_KINDS = {'l1': 0, 'l2': 1, 'laplace': 2}


def head_loss_fwd(x, stats, gamma, beta, w, b, target, loss, kind='l1', crop=None, pred=None, dpred=None, residual=None,
                  res_stride=1, res_off=0, eps=BN_EPS, ab=None):
    """unet_likelihood + regression loss (metrics_model.py:30-132).  x [d0,d1,d2,C]; w [C,K]; target [nvox*n] for n
    regression targets: K = n ('l1', 'l2') or 2n ('laplace': intensities then spreads); crop = (begin[3], size[3]) of the
    loss_cropping box or None; residual [nvox, res_stride] with res_off = the channel (or one per target) added to the
    intensities; pred / dpred [nvox*K].  1 <= K <= 16 (16 l1 / l2 targets, or 8 laplace targets with their spreads)"""
    C = int(x.shape[-1])
    if x.dim() != 4:
        raise ValueError('x should be [d0, d1, d2, C]')
    K = w.numel() // C
    nvox = x.numel() // C
    n = K // 2 if kind == 'laplace' else K
    if w.numel() != C * K or K < 1 or K > 16 or (kind == 'laplace' and K % 2) or target.numel() != nvox * n:
        raise ValueError('head with %d output channels / target of %d values do not fit the %s loss on %d voxels'
                         % (K, target.numel(), kind, nvox))
    shape = _lib.I3(*[int(v) for v in x.shape[:3]])
    box = None
    if crop is not None:
        box = (_lib.c_int * 6)(*([int(v) for v in crop[0]] + [int(v) for v in crop[1]]))
    offs = [int(res_off)] * n if np.ndim(res_off) == 0 else [int(v) for v in res_off]
    if len(offs) != n:
        raise ValueError('one residual channel per regression target is needed (%d given, %d targets)' % (len(offs), n))
    if ab is not None:   # one l1 / l2 target: also the sums head_bwd_from_sums needs, ab [C + 1] (zeroed by the caller)
        if K != 1 or kind == 'laplace' or ab.numel() < C + 1:
            raise ValueError('the fused backward sums exist for the 1-channel l1 / l2 head')
        _lib.check(_sym('synthsr_head_loss_fwd_ab', x)(_lib.ptr(x), shape, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                                      _lib.ptr(w), _lib.ptr(b), _lib.ptr(residual), int(res_stride), offs[0],
                                                      _lib.ptr(target), _lib.ptr(pred), _lib.ptr(dpred), _lib.ptr(loss),
                                                      LOSS_KINDS[kind], box, _lib.ptr(ab), _lib.stream()), 'head_loss_fwd_ab')
        return loss
    offs = (_lib.c_int * 16)(*(offs + [0] * (16 - n)))
    _lib.check(_sym('synthsr_head_loss_fwd', x)(_lib.ptr(x), shape, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                         _lib.ptr(w), _lib.ptr(b), K, _lib.ptr(residual), int(res_stride), offs,
                                         _lib.ptr(target), _lib.ptr(pred), _lib.ptr(dpred), _lib.ptr(loss),
                                         LOSS_KINDS[kind], box, _lib.stream()), 'head_loss_fwd')
    return loss


_SSIM_TAPS = None


def ssim_taps():
    """1-D factor of TensorFlow's `_fspecial_gauss(11, 1.5)` window (softmax of -(x^2+y^2)/(2 sigma^2) = outer product
    of the normalised 1-D Gaussians), float32"""
    global _SSIM_TAPS
    if _SSIM_TAPS is None:
        c = np.arange(11, dtype=np.float32) - np.float32(5)
        g = np.exp(np.square(c) * np.float32(-0.5 / (1.5 * 1.5)), dtype=np.float32)
        _SSIM_TAPS = (g / g.sum(dtype=np.float32)).astype(np.float32)
    return _SSIM_TAPS


SSIM_ORIENTATIONS = (((1, 2), 2.0 / 3.0), ((2, 0), 1.0 / 3.0))  # window axes, weight (metrics_model.py:109-125: xy + xz
# are both slices across axis 0 - the xz transpose only swaps the window axes; yz = slices across axis 1)


def ssim_loss(pred, target, shape, loss, dpred, crop=None, scratch=None):
    """loss += -(1/3)(ssim_xy + ssim_xz + ssim_yz) of SynthSR/metrics_model.py:105-125 and dpred = its gradient w.r.t.
    pred (zero outside the loss_cropping box).  pred, target, dpred: [nvox] of the volume `shape`; crop = (begin[3],
    size[3]) or None; scratch(key, numel) -> float32 device buffer (reused between steps)"""
    lib = _L()
    st = _lib.stream()
    shape = [int(v) for v in shape]
    lo, n = ([0, 0, 0], shape) if crop is None else ([int(v) for v in crop[0]], [int(v) for v in crop[1]])
    if any(n[a] < 11 for a in (0, 1, 2)):
        raise ValueError('the SSIM window needs at least 11 voxels per axis, the loss is evaluated on %s' % (n,))
    if scratch is None:
        cache = {}

        def scratch(key, numel):
            if key not in cache or cache[key].numel() < numel:
                cache[key] = torch.empty(numel, dtype=torch.float32, device=pred.device)
            return cache[key]
    nb = n[0] * n[1] * n[2]
    sh3 = _lib.I3(*shape)
    box = None if crop is None else (_lib.c_int * 6)(*(lo + n))
    taps = (ctypes.c_float * 11)(*[float(v) for v in ssim_taps()])
    maps = scratch('ssim_maps', 4 * nb)
    t1 = scratch('ssim_t1', 4 * nb)
    t2 = scratch('ssim_t2', 4 * nb)
    _lib.check(lib.synthsr_ssim_products(_lib.ptr(pred), _lib.ptr(target), sh3, box, _lib.ptr(maps), st), 'ssim_products')
    dpred.zero_()
    for (a, b), weight in SSIM_ORIENTATIONS:
        sa = list(n)
        sa[a] -= 10
        sab = list(sa)
        sab[b] -= 10
        nq = sab[0] * sab[1] * sab[2]
        _lib.check(lib.synthsr_ssim_filter(_lib.ptr(maps), _lib.ptr(t1), _lib.I3(*n), a, 0, 4, taps, st), 'ssim_filter')
        _lib.check(lib.synthsr_ssim_filter(_lib.ptr(t1), _lib.ptr(t2), _lib.I3(*sa), b, 0, 4, taps, st), 'ssim_filter')
        _lib.check(lib.synthsr_ssim_point(_lib.ptr(t2), nq, 1.0, -weight / nq, _lib.ptr(loss), _lib.ptr(t1), st),
                   'ssim_point')
        _lib.check(lib.synthsr_ssim_filter(_lib.ptr(t1), _lib.ptr(t2), _lib.I3(*sab), b, 1, 3, taps, st), 'ssim_filter')
        _lib.check(lib.synthsr_ssim_filter(_lib.ptr(t2), _lib.ptr(t1), _lib.I3(*sa), a, 1, 3, taps, st), 'ssim_filter')
        _lib.check(lib.synthsr_ssim_combine(_lib.ptr(t1), _lib.ptr(pred), _lib.ptr(target), sh3, box, _lib.ptr(dpred), st),
                   'ssim_combine')
    return loss


def head_bwd_from_sums(ab, gamma, beta, w, dw, db, bn_sums=None):
    """head_bwd (dbn not materialised) from the sums head_loss_fwd(..., ab=...) accumulated: dw, db, bn_sums (+=)"""
    C = int(gamma.numel())
    _lib.check(_L().synthsr_head_bwd_from_sums(_lib.ptr(ab), C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(w), _lib.ptr(dw),
                                               _lib.ptr(db), _lib.ptr(bn_sums), _lib.stream()), 'head_bwd_from_sums')


def head_bwd_multi(dpred, x, stats, gamma, beta, w, dbn, dw, db, eps=BN_EPS):
    """K-channel head backward (2 <= K <= 16): dbn = dpred @ w^T written, dw [C,K] and db [K] accumulated"""
    C = int(x.shape[-1])
    nvox = x.numel() // C
    K = w.numel() // C
    if w.numel() != C * K or K < 2 or K > 16 or dpred.numel() != nvox * K:
        raise ValueError('head_bwd_multi takes a head of 2 to 16 output channels and dpred [nvox * K] (K = %d, dpred of %d '
                         'values on %d voxels)' % (K, dpred.numel(), nvox))
    _lib.check(_sym('synthsr_head_bwd_multi', x)(_lib.ptr(dpred), _lib.ptr(x), nvox, C, K, _lib.ptr(stats), _lib.ptr(gamma),
                                          _lib.ptr(beta), eps, _lib.ptr(w), _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db),
                                          _lib.stream()), 'head_bwd_multi')
    return dbn


def head_bwd(dpred, x, stats, gamma, beta, w, dbn, dw, db, eps=BN_EPS, bn_sums=None):
    """dbn (optional) = dpred (x) w; dw, db +=; bn_sums (optional) += BN-backward channel sums of that gradient"""
    C = int(x.shape[-1])
    nvox = x.numel() // C
    _lib.check(_sym('synthsr_head_bwd_ex', x)(_lib.ptr(dpred), _lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma),
                                       _lib.ptr(beta), eps, _lib.ptr(w), _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db),
                                       _lib.ptr(bn_sums), _lib.stream()), 'head_bwd')
    return dbn


def bn_elu_bwd_head(dpred, whead, y, stats, gamma, sums, dbias=None, out=None, eps=BN_EPS, act=1):
    """bn_elu_bwd for the BN in front of the head: incoming gradient dpred[v]*whead[c] formed on the fly"""
    C = int(y.shape[-1])
    if out is None:
        out = torch.empty_like(y)
    _lib.check(_sym('synthsr_bn_act_bwd_head', y)(_lib.ptr(dpred), _lib.ptr(whead), _lib.ptr(y), _lib.ptr(out),
                                                  _lib.ptr(dbias), y.numel() // C, C, _lib.ptr(stats), _lib.ptr(gamma), eps,
                                                  _lib.ptr(sums), int(act), _lib.stream()), 'bn_act_bwd_head')
    return out


def _seg_fp32_rest(what, x, **rest):
    """the softmax-head kernels take their feature map (or write dbn) as float32 or bfloat16; everything else is float32"""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('%s takes float32 or bfloat16 activations (got %s)' % (what, x.dtype))
    for name, t in rest.items():
        if t is not None and t.dtype != torch.float32:
            raise ValueError('%s: %s stays float32 whatever the activations are (got %s)' % (what, name, t.dtype))


def seg_head_fwd(x, stats, gamma, beta, w, b, probs, eps=BN_EPS):
    """probs [nvox, N] (float32) = softmax(bn(x) @ w + b): head of the frozen segmentation U-Net; x float32 or bfloat16
    (bf16: the tile kernel of the softmax heads, C <= 64 in whole quads; BatchNorm, head and softmax in fp32)"""
    lib = _L()
    C = int(x.shape[-1])
    _seg_fp32_rest('seg_head_fwd', x, stats=stats, gamma=gamma, beta=beta, w=w, b=b, probs=probs)
    N = int(probs.shape[-1])
    if probs.numel() != (x.numel() // C) * N or w.numel() != C * N or b.numel() != N:
        raise ValueError('seg_head_fwd: head [%d, %d] with a bias of %d and posteriors of %d values do not fit %d voxels'
                         % (C, N, b.numel(), probs.numel(), x.numel() // C))
    _lib.check(_sym('synthsr_seg_head_fwd', x)(_lib.ptr(x), x.numel() // C, C, _lib.ptr(stats), _lib.ptr(gamma),
                                               _lib.ptr(beta), eps, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(probs),
                                               _lib.stream()), 'seg_head_fwd')
    return probs


def seg_dice_sums(probs, seg, cls_idx, cls_gt, sums):
    """sums [2K] (zeroed here) <- soft-Dice numerators / denominators of the K merged classes"""
    lib = _L()
    sums.zero_()
    _lib.check(lib.synthsr_seg_dice_sums(_lib.ptr(probs), _lib.ptr(seg), int(probs.shape[0]), int(probs.shape[1]),
                                         _lib.ptr(cls_idx), _lib.ptr(cls_gt), int(cls_gt.numel()), _lib.ptr(sums),
                                         _lib.stream()), 'seg_dice_sums')
    return sums


def seg_dice_bwd(probs, seg, w, cls_idx, cls_gt, sums, scale, dbn):
    """dbn [nvox, C] = d(scale * dice_loss)/d(BatchNorm output in front of the segmentation head); dbn float32, or bfloat16
    for a bf16 segmentation network (computed in fp32, rounded to nearest even at the store)"""
    _seg_fp32_rest('seg_dice_bwd', dbn, probs=probs, w=w, sums=sums)
    _lib.check(_sym('synthsr_seg_dice_bwd', dbn)(_lib.ptr(probs), _lib.ptr(seg), int(probs.shape[0]), int(dbn.shape[-1]),
                                                 int(probs.shape[1]), _lib.ptr(w), _lib.ptr(cls_idx), _lib.ptr(cls_gt),
                                                 int(cls_gt.numel()), _lib.ptr(sums), float(scale), _lib.ptr(dbn),
                                                 _lib.stream()), 'seg_dice_bwd')
    return dbn


def _seg_head_dice_args(what, x, w, b, seg, lut, probs):
    """shared checks of seg_head_dice_fwd / _bwd: float32 activations and head, int32 label map and table, shapes that fit"""
    if x.dim() != 4:
        raise ValueError('x should be [d0, d1, d2, C]')
    C = int(x.shape[-1])
    nvox = x.numel() // C
    N = w.numel() // C
    if w.numel() != C * N or N < 1 or b.numel() != N or seg.numel() != nvox or probs.numel() != nvox * N or lut.numel() < 1:
        raise ValueError('%s: head [%d, %d] with a bias of %d, a label map of %d and posteriors of %d values do not fit %d voxels'
                         % (what, C, N, b.numel(), seg.numel(), probs.numel(), nvox))
    if x.dtype != torch.float32 or w.dtype != torch.float32 or probs.dtype != torch.float32:
        raise ValueError('%s is fp32 only (x is %s)' % (what, x.dtype))
    if seg.dtype != torch.int32 or lut.dtype != torch.int32:
        raise ValueError('%s takes the label map and the lookup table as int32 (got %s, %s)' % (what, seg.dtype, lut.dtype))
    return C, nvox, N


BOUNDARY_DIST_MAX = 5   # the integer boundary rule of seg_boundary_mask is the reference's float rule up to here


def check_boundary_dist(boundary_dist):
    """the boundary distance of the weighted soft Dice as an int in 1 .. 5, or ValueError"""
    if isinstance(boundary_dist, bool) or int(boundary_dist) != boundary_dist or not 1 <= int(boundary_dist) <= BOUNDARY_DIST_MAX:
        raise ValueError('boundary_dist should be an integer from 1 to %d (got %r): beyond it the window holds 3333 voxels or '
                         'more and the integer boundary rule no longer equals the float rule it restates'
                         % (BOUNDARY_DIST_MAX, boundary_dist))
    return int(boundary_dist)


def seg_boundary_mask(seg, lut, N, boundary_dist=3, skip_background=True, mask=None):
    """mask [d0,d1,d2] (int64 holding 64 bits; made here unless given) of the label map seg [d0,d1,d2] (int32 label VALUES):
    bit n of mask[v] = voxel v is a boundary voxel of head channel n, DiceLoss's [avg > 0][avg < 1/3 - 1e-4] with avg the
    'same' average pooling of the one-hot of lut[seg] over (2 boundary_dist + 1)^3 (ext/lab2im/layers.py:1349-1353),
    evaluated exactly in integers.  skip_background (and N > 1): bit 0 stays clear.  1 <= boundary_dist <= 5, N <= 64"""
    if seg.dim() != 3 or seg.dtype != torch.int32 or lut.dtype != torch.int32 or lut.numel() < 1:
        raise ValueError('seg_boundary_mask takes an int32 label map [d0, d1, d2] and an int32 lookup table')
    d = check_boundary_dist(boundary_dist)
    if not 1 <= int(N) <= 64:
        raise ValueError('seg_boundary_mask: one mask bit per head channel, N <= 64 (got %r)' % (N,))
    if mask is None:
        mask = torch.empty(seg.shape, dtype=torch.int64, device=seg.device)
    if mask.dtype != torch.int64 or mask.numel() != seg.numel():
        raise ValueError('seg_boundary_mask: the mask holds one int64 per voxel')
    _lib.check(_L().synthsr_seg_boundary_mask(_lib.ptr(seg), _lib.i3(seg.shape), _lib.ptr(lut), int(lut.numel()), int(N), d,
                                              int(bool(skip_background)), _lib.ptr(mask), _lib.stream()), 'seg_boundary_mask')
    return mask


def _seg_dice_mask(what, mask, nvox):
    if mask is not None and (mask.dtype != torch.int64 or mask.numel() != nvox):
        raise ValueError('%s: the boundary mask holds one int64 per voxel (seg_boundary_mask)' % what)


def seg_head_dice_fwd(x, stats, gamma, beta, w, b, seg, lut, probs, sums, eps=BN_EPS, mask=None, boundary_weights=0.,
                      class_weights=None):
    """trainable softmax head + soft Dice, forward: probs [nvox, N] = softmax(bn(x) @ w + b) written and sums [2N] (zeroed
    here) <- the Dice numerators 2 sum gt p | denominators sum gt^2 + p^2, gt = one-hot of lut[seg] (label values outside
    the table or mapped to -1: no class).  x [d0,d1,d2,C] with C <= 64, N <= 64.  loss = mean(1 - (top + 1e-7) / (bottom +
    1e-7)).
    Weighted (a `mask` of seg_boundary_mask and / or `class_weights` other than None): every term of voxel v and class n
    counts 1 + boundary_weights * (bit n of mask[v]) times, and sums is [3N]: numerators | denominators | the weighted
    volumes sum w gt that dynamic class weights are the inverse of.  The class weights themselves enter the loss,
    sum_n c_n (1 - dice_n), and the backward pass only"""
    C, nvox, N = _seg_head_dice_args('seg_head_dice_fwd', x, w, b, seg, lut, probs)
    weighted = mask is not None or class_weights is not None
    rows = 3 if weighted else 2
    if sums.numel() != rows * N:
        raise ValueError('seg_head_dice_fwd: sums should hold %d N = %d values, holds %d' % (rows, rows * N, sums.numel()))
    sums.zero_()
    if not weighted:
        _lib.check(_L().synthsr_seg_head_dice_fwd(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                                  _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut), int(lut.numel()),
                                                  _lib.ptr(probs), _lib.ptr(sums), _lib.stream()), 'seg_head_dice_fwd')
        return probs
    _seg_dice_mask('seg_head_dice_fwd', mask, nvox)
    _lib.check(_L().synthsr_seg_head_dice_fwd_weighted(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                       eps, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut),
                                                       int(lut.numel()), _lib.ptr(mask), float(boundary_weights),
                                                       _lib.ptr(probs), _lib.ptr(sums), _lib.stream()), 'seg_head_dice_fwd')
    return probs


def seg_head_dice_bwd(probs, seg, lut, x, stats, gamma, beta, w, sums, dbn, dw, db, scale=1.0, eps=BN_EPS, mask=None,
                      boundary_weights=0., class_weights=None):
    """backward of scale * Dice through softmax and head: dbn [d0,d1,d2,C] (gradient w.r.t. the last BatchNorm's output)
    written, dw [C, N] and db [N] accumulated; probs / sums as seg_head_dice_fwd left them.
    Weighted (`mask` and / or `class_weights` given, as in seg_head_dice_fwd; sums [3N]): the gradient of
    scale * sum_n c_n (1 - dice_n), c = class_weights [N] (float32, device; None: 1 / N each), constants of the step"""
    C, nvox, N = _seg_head_dice_args('seg_head_dice_bwd', x, w, db, seg, lut, probs)
    weighted = mask is not None or class_weights is not None
    if sums.numel() != (3 if weighted else 2) * N or dbn.numel() != x.numel() or dw.numel() != C * N or dbn.dtype != torch.float32:
        raise ValueError('seg_head_dice_bwd: sums [2 N] (weighted: [3 N]), dbn like x (float32) and dw [C, N] are needed')
    if not weighted:
        _lib.check(_L().synthsr_seg_head_dice_bwd(_lib.ptr(probs), _lib.ptr(seg), _lib.ptr(lut), int(lut.numel()), _lib.ptr(x),
                                                  nvox, C, N, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.ptr(w),
                                                  _lib.ptr(sums), float(scale), _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db),
                                                  _lib.stream()), 'seg_head_dice_bwd')
        return dbn
    _seg_dice_mask('seg_head_dice_bwd', mask, nvox)
    if class_weights is None:
        class_weights = torch.full((N,), 1.0 / N, dtype=torch.float32, device=x.device)
    if class_weights.dtype != torch.float32 or class_weights.numel() != N or class_weights.device != x.device:
        raise ValueError('seg_head_dice_bwd: class_weights is a float32 device tensor of N = %d values' % N)
    _lib.check(_L().synthsr_seg_head_dice_bwd_weighted(_lib.ptr(probs), _lib.ptr(seg), _lib.ptr(lut), int(lut.numel()),
                                                       _lib.ptr(x), nvox, C, N, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                       eps, _lib.ptr(w), _lib.ptr(sums), _lib.ptr(mask), float(boundary_weights),
                                                       _lib.ptr(class_weights), float(scale), _lib.ptr(dbn), _lib.ptr(dw),
                                                       _lib.ptr(db), _lib.stream()), 'seg_head_dice_bwd')
    return dbn


SEG_LOGIT_LOSSES = {'wl2': 0, 'ce': 1}   # SYNTHSR_SEG_LOSS_WL2 / _CE


def _seg_head_logit_loss_args(what, x, w, b, seg, lut, sums, kind):
    """shared checks of seg_head_logit_loss_fwd / _bwd: those of the soft-Dice head (without posteriors), three sums and a
    known loss"""
    if kind not in SEG_LOGIT_LOSSES:
        raise ValueError('%s: kind should be \'wl2\' or \'ce\' (got %r)' % (what, kind))
    if x.dim() != 4:
        raise ValueError('x should be [d0, d1, d2, C]')
    C = int(x.shape[-1])
    nvox = x.numel() // C
    N = w.numel() // C
    if w.numel() != C * N or N < 1 or b.numel() != N or seg.numel() != nvox or lut.numel() < 1:
        raise ValueError('%s: head [%d, %d] with a bias of %d and a label map of %d values do not fit %d voxels'
                         % (what, C, N, b.numel(), seg.numel(), nvox))
    if any(t.dtype != torch.float32 for t in (x, w, b, sums)):
        raise ValueError('%s is fp32 only (x is %s)' % (what, x.dtype))
    if seg.dtype != torch.int32 or lut.dtype != torch.int32:
        raise ValueError('%s takes the label map and the lookup table as int32 (got %s, %s)' % (what, seg.dtype, lut.dtype))
    if sums.numel() != 3:
        raise ValueError('%s: sums should hold 3 values, holds %d' % (what, sums.numel()))
    return C, nvox, N


def seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, sums, kind, target_value=5., eps=BN_EPS):
    """trainable softmax head + a loss on its LOGITS z = bn(x) @ w + b, forward: sums [3] (zeroed here) accumulated, nothing
    written per voxel.  gt = one-hot of lut[seg] (label values outside the table or mapped to -1: no class).
    kind 'wl2' (WeightedL2Loss, ext/lab2im/layers.py:1408-1412): sums = sum_v a_v sum_n (z - t (2 gt - 1))^2 | voxels not of
    class 0 | voxels of class 0, a_v = 1e-8 on class 0 and 1 elsewhere, t = target_value;
    loss = sums[0] / ((sums[1] + 1e-8 sums[2]) N).
    kind 'ce' (CrossEntropyLoss, :1498-1526, enable_checks=False): sums = sum of -log softmax(z)_k over the voxels with a
    class | their number | unused; loss = sums[0] / nvox.  x [d0,d1,d2,C] with C <= 64, 2 <= N <= 64."""
    C, nvox, N = _seg_head_logit_loss_args('seg_head_logit_loss_fwd', x, w, b, seg, lut, sums, kind)
    sums.zero_()
    _lib.check(_L().synthsr_seg_head_logit_loss_fwd(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps,
                                                    _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut), int(lut.numel()),
                                                    SEG_LOGIT_LOSSES[kind], float(target_value), _lib.ptr(sums), _lib.stream()),
               'seg_head_logit_loss_fwd')
    return sums


def seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums, dbn, dw, db, kind, target_value=5., scale=1.0,
                            eps=BN_EPS):
    """backward of scale * (the loss of seg_head_logit_loss_fwd) through the head: dbn [d0,d1,d2,C] (gradient w.r.t. the last
    BatchNorm's output) written, dw [C, N] and db [N] accumulated; sums as seg_head_logit_loss_fwd left them.  x is read once
    and the logits are formed again: no posteriors are kept between the two calls"""
    C, nvox, N = _seg_head_logit_loss_args('seg_head_logit_loss_bwd', x, w, b, seg, lut, sums, kind)
    if dbn.numel() != x.numel() or dw.numel() != C * N or db.numel() != N or any(t.dtype != torch.float32 for t in (dbn, dw, db)):
        raise ValueError('seg_head_logit_loss_bwd: dbn like x, dw [C, N] and db [N] (float32) are needed')
    _lib.check(_L().synthsr_seg_head_logit_loss_bwd(_lib.ptr(seg), _lib.ptr(lut), int(lut.numel()), _lib.ptr(x), nvox, C, N,
                                                    _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.ptr(w),
                                                    _lib.ptr(b), SEG_LOGIT_LOSSES[kind], float(target_value), _lib.ptr(sums),
                                                    float(scale), _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db), _lib.stream()),
               'seg_head_logit_loss_bwd')
    return dbn


def _seg_head_label_args(what, x, w, b, labels, out):
    """shared checks of seg_head_argmax / _tta_argmax: float32 or bfloat16 activations, a float32 head, int32 label values
    and label map"""
    if x.dim() != 4:
        raise ValueError('x should be [d0, d1, d2, C]')
    C = int(x.shape[-1])
    nvox = x.numel() // C
    N = w.numel() // C
    if w.numel() != C * N or N < 2 or b.numel() != N or labels.numel() != N or out.numel() != nvox:
        raise ValueError('%s: head [%d, %d] with a bias of %d, %d label values and a label map of %d values do not fit %d voxels'
                         % (what, C, N, b.numel(), labels.numel(), out.numel(), nvox))
    _seg_fp32_rest(what, x, w=w, b=b)
    if labels.dtype != torch.int32 or out.dtype != torch.int32:
        raise ValueError('%s takes the label values and writes the label map as int32 (got %s, %s)'
                         % (what, labels.dtype, out.dtype))
    return C, nvox, N


def seg_head_argmax(x, stats, gamma, beta, w, b, labels, out, eps=BN_EPS):
    """out [nvox] (int32) = labels[argmax_n(bn(x) @ w + b)]: the label map of a softmax head without its posteriors (the
    argmax is taken on the logits; equal values: the lowest channel).  x [d0,d1,d2,C] (float32 or bfloat16) with C <= 64,
    2 <= N <= 64; labels [N] int32: head channel -> label value"""
    C, nvox, N = _seg_head_label_args('seg_head_argmax', x, w, b, labels, out)
    _seg_fp32_rest('seg_head_argmax', x, stats=stats, gamma=gamma, beta=beta)
    _lib.check(_sym('synthsr_seg_head_argmax', x)(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                  eps, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(labels), _lib.ptr(out),
                                                  _lib.stream()), 'seg_head_argmax')
    return out


def seg_head_tta_argmax(x, stats, gamma, beta, w, b, labels, prev, perm, out, probs_out=None, eps=BN_EPS):
    """second pass of a flip-averaged segmentation: x [d0,d1,d2,C] is the feature map of the volume flipped along axis 0,
    prev [nvox, N] the posteriors of the unflipped pass, perm [N] int32 the channel permutation swapping left and right
    labels.  p = 0.5 (softmax(bn(x) @ w + b)[perm] + prev[mirrored voxel]); out [nvox] (int32) <- labels[argmax p] and
    probs_out [nvox, N] (optional, not prev) <- p, both at the mirrored voxel: in the frame of the unflipped volume"""
    C, nvox, N = _seg_head_label_args('seg_head_tta_argmax', x, w, b, labels, out)
    if prev.numel() != nvox * N or perm.numel() != N or (probs_out is not None and probs_out.numel() != nvox * N):
        raise ValueError('seg_head_tta_argmax: posteriors [%d, %d] and a permutation of %d channels are needed' % (nvox, N, N))
    if prev.dtype != torch.float32 or perm.dtype != torch.int32 or (probs_out is not None and probs_out.dtype != torch.float32):
        raise ValueError('seg_head_tta_argmax takes float32 posteriors and an int32 permutation')
    _seg_fp32_rest('seg_head_tta_argmax', x, stats=stats, gamma=gamma, beta=beta)
    _lib.check(_sym('synthsr_seg_head_tta_argmax', x)(_lib.ptr(x), _lib.i3(x.shape[:3]), C, _lib.ptr(stats), _lib.ptr(gamma),
                                                      _lib.ptr(beta), eps, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(labels),
                                                      _lib.ptr(prev), _lib.ptr(perm), _lib.ptr(out), _lib.ptr(probs_out),
                                                      _lib.stream()), 'seg_head_tta_argmax')
    return out


def seg_label_counts(a, b, lut, N, counts=None):
    """counts [3, N] (int64, zeroed here) <- per head channel k: voxels with a = b = k | with a = k | with b = k, for two int32
    label maps of equal size; lut (int32): label value -> channel or -1 (values outside the table: no channel).  Exact."""
    if a.dtype != torch.int32 or b.dtype != torch.int32 or lut.dtype != torch.int32:
        raise ValueError('seg_label_counts takes the label maps and the lookup table as int32 (got %s, %s, %s)'
                         % (a.dtype, b.dtype, lut.dtype))
    if a.numel() != b.numel() or a.numel() < 1 or lut.numel() < 1:
        raise ValueError('seg_label_counts: label maps of %d and %d voxels' % (a.numel(), b.numel()))
    N = int(N)
    if counts is None:
        counts = torch.empty(3, N, dtype=torch.int64, device=a.device)
    if counts.numel() != 3 * N or counts.dtype != torch.int64:
        raise ValueError('seg_label_counts: counts should be int64 [3, %d]' % N)
    counts.zero_()
    _lib.check(_L().synthsr_seg_label_counts(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(lut), int(lut.numel()), N,
                                             _lib.ptr(counts), _lib.stream()), 'seg_label_counts')
    return counts


SURFACE_MAX_SIDE = 1024   # include/synthsr_hip.h: synthsr_seg_surface_dist2


def seg_surface_workspace_bytes(shape, N):
    """bytes of device scratch seg_surface_dist2 needs for label maps of `shape` and N head channels"""
    if len(shape) != 3 or not all(1 <= int(s) <= SURFACE_MAX_SIDE for s in shape) or not 1 <= int(N) <= 64:
        raise ValueError('seg_surface_dist2 takes label maps [d0, d1, d2] with sides 1 .. %d and 1 <= N <= 64 (got %s, N = %r)'
                         % (SURFACE_MAX_SIDE, tuple(shape), N))
    return int(_L().synthsr_seg_surface_workspace_bytes(_lib.i3(shape), int(N)))


def seg_surface_dist2(a, b, lut, N, d2_ab=None, d2_ba=None, workspace=None):
    """(d2_ab, d2_ba), int32 of the maps' shape, for two int32 label maps [d0, d1, d2] of equal shape: at a surface voxel of
    class k of `a` (a face neighbour outside the volume or of another class) d2_ab holds the squared distance, in voxels, to the
    nearest surface voxel of class k of `b` (INT32_MAX when b has none), elsewhere -1; d2_ba likewise with the maps exchanged.
    lut (int32): label value -> channel or -1.  Exact integers.  workspace: a uint8 tensor of seg_surface_workspace_bytes()
    (taken from torch when None)."""
    if a.dtype != torch.int32 or b.dtype != torch.int32 or lut.dtype != torch.int32:
        raise ValueError('seg_surface_dist2 takes the label maps and the lookup table as int32 (got %s, %s, %s)'
                         % (a.dtype, b.dtype, lut.dtype))
    if a.dim() != 3 or a.shape != b.shape or lut.numel() < 1:
        raise ValueError('seg_surface_dist2: label maps of shapes %s and %s' % (tuple(a.shape), tuple(b.shape)))
    N = int(N)
    need = seg_surface_workspace_bytes(a.shape, N)
    outs = []
    for name, t in (('d2_ab', d2_ab), ('d2_ba', d2_ba)):
        if t is None:
            t = torch.empty(a.shape, dtype=torch.int32, device=a.device)
        if t.numel() != a.numel() or t.dtype != torch.int32:
            raise ValueError('seg_surface_dist2: %s should be int32 with one value per voxel' % name)
        outs.append(t)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=a.device)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError('seg_surface_dist2: the workspace should be a 16-byte aligned uint8 tensor of at least %d bytes' % need)
    _lib.check(_L().synthsr_seg_surface_dist2(_lib.ptr(a), _lib.ptr(b), _lib.i3(a.shape), _lib.ptr(lut), int(lut.numel()), N,
                                              _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(workspace), workspace.numel(),
                                              _lib.stream()), 'seg_surface_dist2')
    return outs[0], outs[1]


SR_SCORES_MAX_SIDE = 4096   # include/synthsr_hip.h: synthsr_sr_moments / _errors / _ssim3d
SR_SSIM_WINDOW = 11


def sr_scores_workspace_bytes(shape):
    """bytes of device scratch any of sr_moments / sr_errors / sr_ssim3d needs for volumes of `shape`"""
    if len(shape) != 3 or not all(1 <= int(s) <= SR_SCORES_MAX_SIDE for s in shape):
        raise ValueError('the image scores take volumes [d0, d1, d2] with sides 1 .. %d (got %s)' % (SR_SCORES_MAX_SIDE, tuple(shape)))
    return int(_L().synthsr_sr_scores_workspace_bytes(_lib.i3(shape)))


def _sr_scores_args(what, pred, truth, mask, workspace, nout, out, min_side=1):
    for name, t in (('pred', pred), ('truth', truth)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('%s takes %s as a contiguous float32 volume (got %s)' % (what, name, t.dtype))
    if pred.dim() != 3 or pred.shape != truth.shape:
        raise ValueError('%s: volumes of shapes %s and %s' % (what, tuple(pred.shape), tuple(truth.shape)))
    if min(pred.shape) < min_side:
        raise ValueError('%s needs every side >= %d (got %s)' % (what, min_side, tuple(pred.shape)))
    if mask is not None and (mask.dtype != torch.int32 or mask.shape != pred.shape or not mask.is_contiguous()):
        raise ValueError('%s takes the mask as a contiguous int32 volume of the images\' shape' % what)
    need = sr_scores_workspace_bytes(pred.shape)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=pred.device)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError('%s: the workspace should be an 8-byte aligned uint8 tensor of at least %d bytes' % (what, need))
    if out is None:
        out = torch.empty(nout, dtype=torch.float64, device=pred.device)
    if out.dtype != torch.float64 or out.numel() != nout:
        raise ValueError('%s: out should hold %d float64 values' % (what, nout))
    return workspace, out


def sr_moments(pred, truth, mask=None, out=None, workspace=None):
    """float64 device tensor [12]: n, shift_p, shift_t, and over the masked voxels the sums of p', t', p'^2, t'^2, p't'
    (p' = pred - shift_p, t' = truth - shift_t), min / max of pred, min / max of truth (include/synthsr_hip.h)"""
    workspace, out = _sr_scores_args('sr_moments', pred, truth, mask, workspace, 12, out)
    _lib.check(_L().synthsr_sr_moments(_lib.ptr(pred), _lib.ptr(truth), _lib.ptr(mask), _lib.i3(pred.shape), _lib.ptr(out),
                                       _lib.ptr(workspace), workspace.numel(), _lib.stream()), 'sr_moments')
    return out


def sr_errors(pred, truth, mask=None, a=1.0, b=0.0, out=None, workspace=None):
    """float64 device tensor [4]: n, sum |d|, sum d^2, max |d| over the masked voxels, d = a pred + b - truth"""
    workspace, out = _sr_scores_args('sr_errors', pred, truth, mask, workspace, 4, out)
    _lib.check(_L().synthsr_sr_errors(_lib.ptr(pred), _lib.ptr(truth), _lib.ptr(mask), _lib.i3(pred.shape), float(a), float(b),
                                      _lib.ptr(out), _lib.ptr(workspace), workspace.numel(), _lib.stream()), 'sr_errors')
    return out


def sr_ssim3d(pred, truth, mask=None, a=1.0, b=0.0, inv_range=1.0, want_map=False, out=None, ssim_map=None, workspace=None):
    """(float64 device tensor [2]: the sum of the 3-D SSIM (11^3 Gaussian window, sigma 1.5, 'valid' positions) of
    (a pred + b) inv_range against truth inv_range over the positions whose centre voxel is in the mask, and their number;
    the float32 SSIM map [d0 - 10, d1 - 10, d2 - 10] or None)"""
    workspace, out = _sr_scores_args('sr_ssim3d', pred, truth, mask, workspace, 2, out, min_side=SR_SSIM_WINDOW)
    mshape = tuple(int(s) - SR_SSIM_WINDOW + 1 for s in pred.shape)
    if ssim_map is None and want_map:
        ssim_map = torch.empty(mshape, dtype=torch.float32, device=pred.device)
    if ssim_map is not None and (ssim_map.dtype != torch.float32 or tuple(ssim_map.shape) != mshape):
        raise ValueError('sr_ssim3d: the map should be float32 of shape %s' % (mshape,))
    _lib.check(_L().synthsr_sr_ssim3d(_lib.ptr(pred), _lib.ptr(truth), _lib.ptr(mask), _lib.i3(pred.shape), float(a), float(b),
                                      float(inv_range), _lib.ptr(out), _lib.ptr(ssim_map), _lib.ptr(workspace),
                                      workspace.numel(), _lib.stream()), 'sr_ssim3d')
    return out, ssim_map


COMPONENTS_MAX_GROUPS = 64   # include/synthsr_hip.h: synthsr_seg_components
CONNECTIVITIES = (6, 18, 26)


def seg_components_workspace_bytes(shape):
    """bytes of device scratch seg_components and seg_keep_largest need for a label map of `shape`"""
    if len(shape) != 3 or not all(1 <= int(s) <= SURFACE_MAX_SIDE for s in shape):
        raise ValueError('seg_components takes a label map [d0, d1, d2] with sides 1 .. %d (got %s)'
                         % (SURFACE_MAX_SIDE, tuple(shape)))
    return int(_L().synthsr_seg_components_workspace_bytes(_lib.i3(shape)))


def _seg_components_args(what, labels, lut, G, workspace):
    if labels.dtype != torch.int32 or lut.dtype != torch.int32:
        raise ValueError('%s takes the label map and the lookup table as int32 (got %s, %s)' % (what, labels.dtype, lut.dtype))
    if labels.dim() != 3 or lut.numel() < 1:
        raise ValueError('%s: a label map [d0, d1, d2] and a lookup table of at least one entry, got shapes %s and %s'
                         % (what, tuple(labels.shape), tuple(lut.shape)))
    need = seg_components_workspace_bytes(labels.shape)
    if not 1 <= int(G) <= COMPONENTS_MAX_GROUPS:
        raise ValueError('%s: 1 <= G <= %d groups (got %r)' % (what, COMPONENTS_MAX_GROUPS, G))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=labels.device)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError('%s: the workspace should be a 16-byte aligned uint8 tensor of at least %d bytes' % (what, need))
    return workspace


def seg_components(labels, lut, G, connectivity=6, comp=None, workspace=None):
    """comp, int32 of the map's shape, for an int32 label map [d0, d1, d2]: the smallest linear index of any voxel of the voxel's
    connected component, -1 for a voxel in no group.  lut (int32): label value -> group 0 .. G-1 or -1; voxels are connected
    when they are in the same group and adjacent under `connectivity` (6: faces, 18: and edges, 26: and corners).  Exact and
    unique.  workspace: a uint8 tensor of seg_components_workspace_bytes() (taken from torch when None)."""
    workspace = _seg_components_args('seg_components', labels, lut, G, workspace)
    if connectivity not in CONNECTIVITIES:
        raise ValueError('seg_components: connectivity is 6, 18 or 26 (got %r)' % (connectivity,))
    if comp is None:
        comp = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    if comp.numel() != labels.numel() or comp.dtype != torch.int32:
        raise ValueError('seg_components: comp should be int32 with one value per voxel')
    _lib.check(_L().synthsr_seg_components(_lib.ptr(labels), _lib.i3(labels.shape), _lib.ptr(lut), int(lut.numel()), int(G),
                                           int(connectivity), _lib.ptr(comp), _lib.ptr(workspace), workspace.numel(),
                                           _lib.stream()), 'seg_components')
    return comp


def seg_keep_largest(labels, comp, lut, G, fill_value, out=None, stats=None, workspace=None):
    """(out, stats) for an int32 label map and its component map (seg_components with the same lut and G): out holds fill_value
    at every voxel whose component is not the largest of its group (of several of that size: the one with the smallest root),
    the label value elsewhere, voxels in no group included; out may be `labels`.  stats, int64 [G, 4]: root of the kept
    component (-1: empty group), its size, the components and the voxels of the group."""
    workspace = _seg_components_args('seg_keep_largest', labels, lut, G, workspace)
    G = int(G)
    if comp.dtype != torch.int32 or comp.numel() != labels.numel():
        raise ValueError('seg_keep_largest: comp should be int32 with one value per voxel')
    if not -2 ** 31 <= int(fill_value) < 2 ** 31:
        raise ValueError('seg_keep_largest: fill_value should fit int32 (got %r)' % (fill_value,))
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    if out.numel() != labels.numel() or out.dtype != torch.int32:
        raise ValueError('seg_keep_largest: out should be int32 with one value per voxel')
    if stats is None:
        stats = torch.empty(G, 4, dtype=torch.int64, device=labels.device)
    if stats.numel() != 4 * G or stats.dtype != torch.int64:
        raise ValueError('seg_keep_largest: stats should be int64 [%d, 4]' % G)
    _lib.check(_L().synthsr_seg_keep_largest(_lib.ptr(labels), _lib.ptr(comp), _lib.i3(labels.shape), _lib.ptr(lut),
                                             int(lut.numel()), G, int(fill_value), _lib.ptr(out), _lib.ptr(stats),
                                             _lib.ptr(workspace), workspace.numel(), _lib.stream()), 'seg_keep_largest')
    return out, stats


def seg_resample_argmax(probs, box, M, out_shape, labels, fill_value, want_probs=False, out=None, probs_out=None):
    """The label map on another voxel grid, from posteriors: `out`, int32 of `out_shape`, and with want_probs also the
    interpolated posteriors, float32 [*out_shape, N].  probs: float32 [s0, s1, s2, N] (channel last); box: (lo0, lo1, lo2, hi0,
    hi1, hi2), inclusive, the part of the source that holds the volume; M: 3 x 4 (or 4 x 4) float64 on the host, output voxel
    index -> source voxel coordinates; labels: int32 [N], channel -> label value.  A voxel that M maps more than half a voxel
    outside the box gets fill_value and zero posteriors; the others the label of the largest trilinearly interpolated posterior,
    the lowest channel on equal values (include/synthsr_hip.h: synthsr_seg_resample_argmax)."""
    if probs.dtype != torch.float32 or labels.dtype != torch.int32:
        raise ValueError('seg_resample_argmax takes the posteriors as float32 and the label values as int32 (got %s, %s)'
                         % (probs.dtype, labels.dtype))
    if probs.dim() != 4 or not all(1 <= int(s) <= SURFACE_MAX_SIDE for s in probs.shape[:3]):
        raise ValueError('seg_resample_argmax: posteriors [s0, s1, s2, N] with sides 1 .. %d, got shape %s'
                         % (SURFACE_MAX_SIDE, tuple(probs.shape)))
    N = int(probs.shape[3])
    if not 2 <= N <= 64 or labels.numel() != N:
        raise ValueError('seg_resample_argmax: 2 <= N <= 64 channels and one label value per channel (got N = %d, %d label values)'
                         % (N, labels.numel()))
    out_shape = tuple(int(s) for s in out_shape)
    if len(out_shape) != 3 or not all(1 <= s <= SURFACE_MAX_SIDE for s in out_shape):
        raise ValueError('seg_resample_argmax: out_shape [d0, d1, d2] with sides 1 .. %d, got %s' % (SURFACE_MAX_SIDE, out_shape))
    box = [int(b) for b in np.asarray(box).reshape(-1)]
    if len(box) != 6 or not all(0 <= box[a] <= box[3 + a] < int(probs.shape[a]) for a in range(3)):
        raise ValueError('seg_resample_argmax: box (lo0, lo1, lo2, hi0, hi1, hi2) with 0 <= lo <= hi inside the source %s, got %s'
                         % (tuple(probs.shape[:3]), box))
    M = np.asarray(M, dtype=np.float64)
    if M.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(M)):
        raise ValueError('seg_resample_argmax: M should be a finite 3 x 4 (or 4 x 4) matrix')
    M = np.ascontiguousarray(M[:3])
    if not -2 ** 31 <= int(fill_value) < 2 ** 31:
        raise ValueError('seg_resample_argmax: fill_value should fit int32 (got %r)' % (fill_value,))
    nvox = out_shape[0] * out_shape[1] * out_shape[2]
    if out is None:
        out = torch.empty(out_shape, dtype=torch.int32, device=probs.device)
    if out.numel() != nvox or out.dtype != torch.int32:
        raise ValueError('seg_resample_argmax: out should be int32 with one value per output voxel')
    if want_probs and probs_out is None:
        probs_out = torch.empty(out_shape + (N,), dtype=torch.float32, device=probs.device)
    if probs_out is not None and (probs_out.numel() != nvox * N or probs_out.dtype != torch.float32):
        raise ValueError('seg_resample_argmax: probs_out should be float32 [%d, %d, %d, %d]' % (out_shape + (N,)))
    _lib.check(_L().synthsr_seg_resample_argmax(_lib.ptr(probs), _lib.i3(probs.shape[:3]), N, (ctypes.c_int * 6)(*box),
                                                M.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.i3(out_shape),
                                                _lib.ptr(labels), int(fill_value), _lib.ptr(out), _lib.ptr(probs_out),
                                                _lib.stream()), 'seg_resample_argmax')
    return (out, probs_out) if (want_probs or probs_out is not None) else out


VOLUME_MAX_SIDE = 1024      # include/synthsr_hip.h: "inference volumes"
VOLUME_MAX_RADIUS = 16
VOLUME_RESAMPLE_WORKSPACE_BYTES = 8192
RESAMPLE_MODES = ('clamp', 'zero_outside')   # index = SYNTHSR_RESAMPLE_*


def _volume_f32(what, name, t, dims=(3,)):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s takes %s as a contiguous float32 tensor (got %s)' % (what, name, getattr(t, 'dtype', type(t))))
    if t.dim() not in dims or not all(1 <= int(s) <= VOLUME_MAX_SIDE for s in t.shape[:3]):
        raise ValueError('%s: %s should be [d0, d1, d2]%s with sides 1 .. %d, got shape %s'
                         % (what, name, ' or [d0, d1, d2, C]' if 4 in dims else '', VOLUME_MAX_SIDE, tuple(t.shape)))
    return t


def _volume_sides(what, name, shape):
    shape = tuple(int(s) for s in np.asarray(shape).reshape(-1))
    if len(shape) != 3 or not all(1 <= s <= VOLUME_MAX_SIDE for s in shape):
        raise ValueError('%s: %s [d0, d1, d2] with sides 1 .. %d, got %s' % (what, name, VOLUME_MAX_SIDE, shape))
    return shape


def _volume_box(what, buf, channel, offset, shape):
    """(Cd, offset) of a box of `shape` at `offset` in channel `channel` of buf [D0, D1, D2] or [D0, D1, D2, Cd]"""
    Cd = int(buf.shape[3]) if buf.dim() == 4 else 1
    if not 1 <= Cd <= 2 or not 0 <= int(channel) < Cd:
        raise ValueError('%s: a buffer of 1 or 2 channels and a channel inside it (got %d channels, channel %r)' % (what, Cd, channel))
    offset = tuple(int(o) for o in np.asarray(offset).reshape(-1))
    if len(offset) != 3 or not all(0 <= offset[a] <= int(buf.shape[a]) - shape[a] for a in range(3)):
        raise ValueError('%s: the box of shape %s at offset %s does not lie inside the buffer %s'
                         % (what, shape, offset, tuple(buf.shape[:3])))
    return Cd, offset


def volume_blur_axis(x, axis, taps, out=None):
    """One axis of scipy.ndimage.gaussian_filter(mode='reflect') on a float32 volume [n0, n1, n2]: out[i] = sum_t taps[t + r]
    x[reflect(i + t)] along `axis`.  taps: 2 r + 1 values (host; volumes.gaussian_taps), 1 <= r <= 16.  out may not be x."""
    _volume_f32('volume_blur_axis', 'x', x)
    if axis not in (0, 1, 2):
        raise ValueError('volume_blur_axis: axis is 0, 1 or 2 (got %r)' % (axis,))
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
    r = (len(taps) - 1) // 2
    if len(taps) != 2 * r + 1 or not 1 <= r <= VOLUME_MAX_RADIUS or not np.all(np.isfinite(taps)):
        raise ValueError('volume_blur_axis: taps are 2 r + 1 finite values with 1 <= r <= %d (got %d values)'
                         % (VOLUME_MAX_RADIUS, len(taps)))
    if out is None:
        out = torch.empty_like(x)
    _volume_f32('volume_blur_axis', 'out', out)
    if out.shape != x.shape or out.device != x.device or out.data_ptr() == x.data_ptr():
        raise ValueError('volume_blur_axis: out should be another float32 volume of x\'s shape on its device')
    _lib.check(_L().synthsr_volume_blur_axis(_lib.ptr(x), _lib.i3(x.shape), int(axis),
                                             taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r, _lib.ptr(out), _lib.stream()),
               'volume_blur_axis')
    return out


def volume_resample(src, M, out_shape, mode='clamp', out=None, offset=(0, 0, 0), channel=0, minmax=None, workspace=None):
    """(out, minmax): trilinear samples of the float32 volume src [s0, s1, s2] at pos = M (i, j, k, 1) for every voxel (i, j, k) of
    out_shape, written to out[offset + (i, j, k)] (out [D0, D1, D2]) or out[offset + (i, j, k), channel] (out [D0, D1, D2, Cd],
    Cd <= 2); the rest of out is left alone.  M: 3 x 4 (or 4 x 4) float64 on the host.  mode 'clamp': positions are clipped to the
    source grid (volumes.resample_volume); 'zero_outside': 0 for positions outside it (volumes.resample_volume_like).  minmax:
    float32 [2] on the device, the minimum and maximum of what was written.  out=None: a new volume of out_shape."""
    what = 'volume_resample'
    _volume_f32(what, 'src', src)
    if mode not in RESAMPLE_MODES:
        raise ValueError('%s: mode is one of %s (got %r)' % (what, RESAMPLE_MODES, mode))
    out_shape = _volume_sides(what, 'out_shape', out_shape)
    M = np.asarray(M, dtype=np.float64)
    if M.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(M)):
        raise ValueError('%s: M should be a finite 3 x 4 (or 4 x 4) matrix' % what)
    M = np.ascontiguousarray(M[:3])
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    _volume_f32(what, 'out', out, dims=(3, 4))
    Cd, offset = _volume_box(what, out, channel, offset, out_shape)
    if minmax is None:
        minmax = torch.empty(2, dtype=torch.float32, device=src.device)
    if minmax.dtype != torch.float32 or minmax.numel() != 2:
        raise ValueError('%s: minmax should hold 2 float32 values' % what)
    if workspace is None:
        workspace = torch.empty(VOLUME_RESAMPLE_WORKSPACE_BYTES, dtype=torch.uint8, device=src.device)
    if workspace.dtype != torch.uint8 or workspace.numel() < VOLUME_RESAMPLE_WORKSPACE_BYTES or workspace.data_ptr() % 4:
        raise ValueError('%s: the workspace should be a 4-byte aligned uint8 tensor of at least %d bytes'
                         % (what, VOLUME_RESAMPLE_WORKSPACE_BYTES))
    if not (out.device == minmax.device == workspace.device == src.device):
        raise ValueError('%s: src, out, minmax and the workspace should be on one device' % what)
    _lib.check(_L().synthsr_volume_resample(_lib.ptr(src), _lib.i3(src.shape), M.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            RESAMPLE_MODES.index(mode), _lib.i3(out_shape), _lib.ptr(out), _lib.i3(out.shape[:3]),
                                            Cd, _lib.i3(offset), int(channel), _lib.ptr(minmax), _lib.ptr(workspace),
                                            workspace.numel(), _lib.stream()), what)
    return out, minmax


def volume_normalise_pad(out, offset, box_shape, minmax, gain=1.0, channel=0):
    """In place on out [D0, D1, D2] or channel `channel` of out [D0, D1, D2, Cd]: x <- gain (x - lo) / (hi - lo) inside the box of
    box_shape at offset, with (lo, hi) = minmax (float32 [2] on the device: volume_resample's), exact 0 outside it whatever the
    buffer held.  hi == lo gives 0 everywhere (the host path gives NaN)."""
    what = 'volume_normalise_pad'
    _volume_f32(what, 'out', out, dims=(3, 4))
    box_shape = _volume_sides(what, 'box_shape', box_shape)
    Cd, offset = _volume_box(what, out, channel, offset, box_shape)
    if not torch.is_tensor(minmax) or minmax.dtype != torch.float32 or minmax.numel() != 2 or minmax.device != out.device:
        raise ValueError('%s: minmax should hold 2 float32 values on the buffer\'s device' % what)
    if not np.isfinite(gain):
        raise ValueError('%s: gain should be finite (got %r)' % (what, gain))
    _lib.check(_L().synthsr_volume_normalise_pad(_lib.ptr(out), _lib.i3(out.shape[:3]), Cd, _lib.i3(offset), _lib.i3(box_shape),
                                                 int(channel), _lib.ptr(minmax), float(gain), _lib.stream()), what)
    return out


def sr_postprocess(net, offset, shape, netf=None, addend=None, a=1.0, b=0.0, lo=-np.inf, hi=np.inf, out=None):
    """out [shape] = clip(a (p + addend) + b, lo, hi) on the box of `shape` at `offset` of the network output net [D0, D1, D2]:
    p = net, or with netf (the output for the volume flipped along axis 0) p = 0.5 net + 0.5 flip0(netf).  addend: None, or a
    float32 tensor of `shape`, any positive strides (a box of a larger buffer as it lies)."""
    what = 'sr_postprocess'
    _volume_f32(what, 'net', net)
    shape = _volume_sides(what, 'shape', shape)
    _, offset = _volume_box(what, net, 0, offset, shape)
    if netf is not None:
        _volume_f32(what, 'netf', netf)
        if netf.shape != net.shape or netf.device != net.device:
            raise ValueError('%s: netf should have net\'s shape and device' % what)
    strides = None
    if addend is not None:
        if (not torch.is_tensor(addend) or addend.dtype != torch.float32 or tuple(addend.shape) != shape
                or addend.device != net.device or min(addend.stride()) < 1):
            raise ValueError('%s: addend should be a float32 tensor of shape %s with positive strides on net\'s device' % (what, shape))
        strides = (ctypes.c_int64 * 3)(*addend.stride())
    if not all(np.isfinite(v) for v in (a, b)) or not lo <= hi:
        raise ValueError('%s: a and b finite and lo <= hi (got a %r, b %r, [%r, %r])' % (what, a, b, lo, hi))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=net.device)
    _volume_f32(what, 'out', out)
    if tuple(out.shape) != shape or out.device != net.device:
        raise ValueError('%s: out should be a float32 volume of shape %s on net\'s device' % (what, shape))
    _lib.check(_L().synthsr_sr_postprocess(_lib.ptr(net), _lib.ptr(netf), _lib.i3(net.shape), _lib.i3(offset), _lib.i3(shape),
                                           None if addend is None else ctypes.c_void_p(addend.data_ptr()), strides, float(a),
                                           float(b), float(lo), float(hi), _lib.ptr(out), _lib.stream()), what)
    return out


def adam_step(p, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
    lib = _L()
    _lib.check(lib.synthsr_adam_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), p.numel(), float(lr_t),
                                     float(beta1), float(beta2), float(eps), float(grad_scale), _lib.stream()),
               'adam_step')


# ---------------------------------------------------------------------- WGAN-GP critic pieces (csrc/critic.hip)
def leaky_relu(x, alpha=0.2, out=None):
    """LeakyReLU (in place when out is None)"""
    out = x if out is None else out
    _lib.check(_L().synthsr_leaky_relu(_lib.ptr(x), None, _lib.ptr(out), x.numel(), float(alpha), _lib.stream()), 'leaky_relu')
    return out


def leaky_relu_bwd(dy, y, alpha=0.2, out=None):
    """dx = dy * (y > 0 ? 1 : alpha); y = the LeakyReLU output"""
    out = torch.empty_like(dy) if out is None else out
    _lib.check(_L().synthsr_leaky_relu(_lib.ptr(y), _lib.ptr(dy), _lib.ptr(out), y.numel(), float(alpha), _lib.stream()),
               'leaky_relu_bwd')
    return out


def dense_fwd(x, W, b, out=None):
    """y [n_out] = b + x [n_in] . W [n_in, n_out]"""
    n_in, n_out = int(W.shape[0]), int(W.shape[1])
    out = torch.empty(n_out, dtype=torch.float32, device=x.device) if out is None else out
    _lib.check(_L().synthsr_dense_fwd(_lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(out), n_in, n_out, _lib.stream()),
               'dense_fwd')
    return out


def dense_bwd(x, W, dy, dx=None, dW=None):
    """dx [n_in] = W dy (written, if given); dW += x (x) dy (if given)"""
    n_in, n_out = int(W.shape[0]), int(W.shape[1])
    _lib.check(_L().synthsr_dense_bwd(_lib.ptr(x), _lib.ptr(W), _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(dW), n_in, n_out,
                                      _lib.stream()), 'dense_bwd')
    return dx


def axpby(x, y, a, b, out=None):
    out = torch.empty_like(x) if out is None else out
    _lib.check(_L().synthsr_axpby(_lib.ptr(x), _lib.ptr(y), _lib.ptr(out), x.numel(), float(a), float(b), _lib.stream()),
               'axpby')
    return out


def sumsq(x, out):
    """out[0] += sum x^2"""
    _lib.check(_L().synthsr_sumsq(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.stream()), 'sumsq')
    return out


def bias_leaky_relu(x, bias, alpha=0.2, out=None):
    out = x if out is None else out
    C = int(x.shape[-1])
    _lib.check(_L().synthsr_bias_leaky_relu(_lib.ptr(x), _lib.ptr(bias), _lib.ptr(out), x.numel(), C, float(alpha),
                                            _lib.stream()), 'bias_leaky_relu')
    return out


def colsum(x, out):
    """out [C] += column sums of x [..., C]"""
    C = int(x.shape[-1])
    _lib.check(_L().synthsr_colsum(_lib.ptr(x), x.numel() // C, C, _lib.ptr(out), _lib.stream()), 'colsum')
    return out


# stride-2 'same' Conv3D (even sizes) on the parity kernels of the folded decoder conv; weights [3,3,3,Cin,Cout]
def pack_stride2_weights(w, lo_shape, mode=0, out=None):
    """mode 0: forward weights, mode 1: data-gradient weights (lo_shape = OUTPUT spatial shape)"""
    return pack_conv_weights_ex(w, lo_shape, 0, int(w.shape[3]), mode, up=2, out=out)


def conv3d_stride2(x, wpacked8, Cout, out=None):
    """x [2a,2b,2c,Cin] -> [a,b,c,Cout] (no bias / activation): y[o] = sum_t w[t] x[2o + t]"""
    lib = _L()
    s = x.shape
    lo_shape = (s[0] // 2, s[1] // 2, s[2] // 2)
    if out is None:
        out = torch.empty(lo_shape + (Cout,), dtype=torch.float32, device=x.device)
    _lib.check(lib.synthsr_conv3d_up_dgrad(conv_ctx(), _lib.ptr(x), _lib.ptr(wpacked8), _lib.ptr(out), _lib.i3(lo_shape), int(Cout),
                                           int(s[3]), _lib.stream()), 'conv3d_stride2')
    return out


def conv3d_stride2_dgrad(dy, wpacked8d, Cin, out=None):
    """dy [a,b,c,Cout] -> gradient w.r.t. the stride-2 conv's input [2a,2b,2c,Cin]"""
    lib = _L()
    s = dy.shape
    if out is None:
        out = torch.empty((2 * s[0], 2 * s[1], 2 * s[2], Cin), dtype=torch.float32, device=dy.device)
    _lib.check(lib.synthsr_conv3d_up_fwd(conv_ctx(), _lib.ptr(dy), _lib.ptr(wpacked8d), None, None, _lib.ptr(out), _lib.i3(s[:3]),
                                         int(s[3]), int(Cin), 0, _lib.stream()), 'conv3d_stride2_dgrad')
    return out


def conv3d_stride2_wgrad(x, dy, dw, dwc, dbias=None):
    """dw [3,3,3,Cin,Cout] += sum_o x[2o + t] (x) dy[o]; dwc: scratch [8,27,Cout,Cin] (zeroed here); dbias += sum dy"""
    lib = _L()
    Ci, Co = int(x.shape[3]), int(dy.shape[3])
    dwc.zero_()
    _check_wgrad(lambda: lib.synthsr_conv3d_up_wgrad(conv_ctx(), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dwc), _lib.i3(dy.shape[:3]), Co, Ci,
                                           _lib.stream()), 'conv3d_stride2_wgrad')
    _lib.check(lib.synthsr_conv3d_stride_unpack(_lib.ptr(dwc), _lib.ptr(dw), Ci, Co, _lib.stream()), 'stride_unpack')
    if dbias is not None:
        colsum(dy, dbias)
    return dw


def mul(x, y, out=None):
    out = torch.empty_like(x) if out is None else out
    _lib.check(_L().synthsr_mul(_lib.ptr(x), _lib.ptr(y), _lib.ptr(out), x.numel(), _lib.stream()), 'mul')
    return out


def lut_gather(labels, lut, out=None):
    """out = lut[labels] (float32; ConvertLabels of the reference): labels int32, lut float32 device tensors"""
    out = torch.empty(labels.shape, dtype=torch.float32, device=labels.device) if out is None else out
    _lib.check(_L().synthsr_lut_gather(_lib.ptr(labels), _lib.ptr(lut), lut.numel(), _lib.ptr(out), labels.numel(),
                                       _lib.stream()), 'lut_gather')
    return out


# ---------------------------------------------------------------------- bf16 convolutions (csrc/conv_bf16.hip)
_bf16_scratch = {}


def pack_conv_weights_bf16(w, mode=0, ci_off=0, cin=None, out=None, up=False):
    """fp32 Keras kernel w [3,3,3,Cin_total,Cout] -> bf16 MFMA fragments (mode 0 forward, 1 data gradient); up: the 8 parity
    sets of the nearest-upsample folding, back to back (conv3d_up / conv3d_up_dgrad)"""
    lib = _L()
    cin_total, cout = int(w.shape[3]), int(w.shape[4])
    cin = cin_total if cin is None else int(cin)
    parities = list(range(8)) if up else [-1]
    n = lib.synthsr_conv3d_bf16_pack_ex(None, None, cin_total, int(ci_off), cin, cout, int(mode), parities[0], None)
    if n < 0:
        _lib.check(int(n), 'conv3d_bf16_pack(size)')
    if out is None:
        out = torch.empty(n * len(parities), dtype=torch.bfloat16, device=w.device)
    assert out.numel() == n * len(parities) and out.dtype == torch.bfloat16
    for k, par in enumerate(parities):
        r = lib.synthsr_conv3d_bf16_pack_ex(_lib.ptr(w), _lib.ptr(out[k * n:(k + 1) * n]), cin_total, int(ci_off), cin, cout,
                                            int(mode), par, _lib.stream())
        if r < 0:
            _lib.check(int(r), 'conv3d_bf16_pack')
    return out


def conv3d_bf16(x, wpacked, bias, Cout, act=1, below=None, stats=None, out=None, alpha=0.0):
    """act(conv3(x) + bias) on bf16 NDHWC tensors (fp32 accumulation); act 2: times ELU'(below); act 3: LeakyReLU(alpha);
    act 4: times LeakyReLU'(below); stats: fp32 [2*Cout] receives the batch mean | variance of the output"""
    lib = _L()
    s = x.shape
    assert x.dtype == torch.bfloat16 and wpacked.dtype == torch.bfloat16
    if out is None:
        out = torch.empty((s[0], s[1], s[2], Cout), dtype=torch.bfloat16, device=x.device)
    nscr = int(lib.synthsr_conv3d_bf16_stats_scratch(_lib.i3(s[:3]), int(s[3]), int(Cout)))
    scratch = _bf16_scratch.get(x.device)   # statistics partials / split-K partial sums (stream-ordered reuse)
    if scratch is None or scratch.numel() < nscr:
        scratch = _bf16_scratch[x.device] = torch.empty(max(nscr, 1 << 20), dtype=torch.float32, device=x.device)
    nscr = scratch.numel()
    with _Timed('conv3d_bf16', s[:3], s[3], Cout):
        _lib.check(lib.synthsr_conv3d_bf16_fwd_ex(_lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out),
                                                  _lib.i3(s[:3]), int(s[3]), int(Cout), int(act), float(alpha),
                                                  _lib.ptr(below), _lib.ptr(stats), _lib.ptr(scratch), nscr,
                                                  _lib.stream()), 'conv3d_bf16_fwd')
    return out


def subsample_odd_bf16(x, below=None, alpha=0.0, out=None):
    """out[o] = x[2 o + 1] (* LeakyReLU'(below[o])): a stride-2 'same' conv = the stride-1 conv at the odd positions"""
    s = x.shape
    lo = (s[0] // 2, s[1] // 2, s[2] // 2)
    if out is None:
        out = torch.empty(lo + (s[3],), dtype=torch.bfloat16, device=x.device)
    _lib.check(_L().synthsr_bf16_subsample_odd(_lib.ptr(x), _lib.ptr(out), _lib.ptr(below), _lib.i3(lo), int(s[3]),
                                               float(alpha), _lib.stream()), 'bf16_subsample_odd')
    return out


def zero_insert_odd_bf16(x, out=None):
    """transpose of subsample_odd_bf16: [2 d0, 2 d1, 2 d2, C] with x at the odd positions, zero elsewhere"""
    s = x.shape
    if out is None:
        out = torch.empty((2 * s[0], 2 * s[1], 2 * s[2], s[3]), dtype=torch.bfloat16, device=x.device)
    _lib.check(_L().synthsr_bf16_zero_insert_odd(_lib.ptr(x), _lib.ptr(out), _lib.i3(s[:3]), int(s[3]), _lib.stream()),
               'bf16_zero_insert_odd')
    return out


def conv3d_wgrad_bf16(x, dz, dw, dbias=None):
    """dw [3,3,3,Cin,Cout] fp32 += weight gradient of bf16 x / dz (dbias += column sums of dz)"""
    lib = _L()
    s = x.shape
    assert x.dtype == torch.bfloat16 and dz.dtype == torch.bfloat16 and dw.dtype == torch.float32
    with _Timed('conv3d_bf16_wgrad', s[:3], s[3], dz.shape[3]):
        _check_wgrad(lambda: lib.synthsr_conv3d_bf16_wgrad(_lib.ptr(x), _lib.ptr(dz), _lib.ptr(dw), _lib.ptr(dbias), _lib.i3(s[:3]),
                                                 int(dw.shape[3]), 0, int(s[3]), int(dz.shape[3]), _lib.stream()),
                   'conv3d_bf16_wgrad')
    return dw


def to_bf16_pad(x, Cd, out=None):
    """fp32 [..., Cs] -> bf16 [..., Cd] with zero-filled extra channels"""
    lib = _L()
    Cs = int(x.shape[-1])
    n = x.numel() // Cs
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (Cd,), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.synthsr_f32_to_bf16_pad(_lib.ptr(x), _lib.ptr(out), n, Cs, int(Cd), _lib.stream()), 'f32_to_bf16_pad')
    return out
