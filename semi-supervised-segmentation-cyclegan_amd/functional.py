"""Host-side operators: torch tensors in, libsscg.so kernels underneath.

Two layers:
  * raw ops (`conv2d_fwd`, `norm_stats`, ...) - thin wrappers over the C ABI (include/sscg.h) that
    allocate outputs through torch's caching allocator and launch on torch's current HIP stream;
  * `torch.autograd.Function`s (`Conv2dFn`, `NormActFn`, ...) that give those kernels the semantics
    of the stock torch.nn modules the reference composes (arch/ops.py:40-57, model.py:268-273).

Tensors keep the reference's logical NCHW shapes; physically they are channels-last (NHWC), which is
what every kernel assumes.  There is no fallback: a non-HIP tensor raises.
"""
import ctypes as C
import math
import os
import weakref

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, PAD_ZEROS, PAD_REFLECT, ConvDesc, check, lib

CL = torch.channels_last


# ----------------------------------------------------------------------------- plumbing
_raw_stream = torch._C._cuda_getCurrentRawStream     # the handle only: torch.cuda.current_stream() builds a Stream object (~6 us)
_cur_dev = getattr(torch._C, "_cuda_getDevice", torch.cuda.current_device)     # the binding itself: torch.cuda.current_device() adds a lazy-init check per call


def _stream():
    return _raw_stream(_cur_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


F32, BF16, BF16X3 = _lib.F32, _lib.BF16, _lib.BF16X3
_DT = {torch.float32: F32, torch.bfloat16: BF16}


def _need_hip(t, f32_only=False):
    if not t.is_cuda:
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % t.device)
    if t.dtype != torch.float32 and (f32_only or t.dtype != torch.bfloat16):
        raise _lib.SscgError("%s tensor expected, got %s" % ("fp32" if f32_only else "fp32 or bf16", t.dtype))


def _dt(t):
    return _DT[t.dtype]


def _same_dtype(*ts):
    d = ts[0].dtype
    for t in ts[1:]:
        if t is not None and t.dtype != d:
            raise _lib.SscgError("operands of one element type expected, got %s and %s" % (d, t.dtype))
    return _DT[d]


class _Workspace:
    """One growable scratch buffer per (device, stream): reuse is ordered by the stream it is used on."""

    def __init__(self):
        self.buf = {}

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 16)
        key = (device, _raw_stream(device.index if device.index is not None else _cur_dev()))
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


_WS = _Workspace()

_HIPRT = []


def _hip_runtime():
    """The HIP runtime torch itself loaded (a second copy's stream handles would be foreign to torch): its path is taken from this
    process's own mappings; None when it cannot be found or lacks the symbol."""
    import ctypes
    if not _HIPRT:
        h = None
        try:
            path = None
            with open("/proc/self/maps") as f:
                for line in f:
                    if "libamdhip64.so" in line:
                        path = line.split(None, 5)[-1].strip()
                        break
            if path is not None:
                h = ctypes.CDLL(path)       # already mapped: dlopen returns the loaded library
                h.hipStreamCreateWithPriority.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint, ctypes.c_int]
                h.hipStreamCreateWithPriority.restype = ctypes.c_int
        except (OSError, AttributeError):
            h = None
        _HIPRT.append(h)
    return _HIPRT[0]


def _make_stream(device, priority=0):
    """A HIP stream of the given priority (HIP's scale: -1 high, 0 normal, 1 low).  torch only creates normal / high priority
    streams; a LOW priority one comes from hipStreamCreateWithPriority and is wrapped (it lives as long as the process).  Where
    that is not possible (runtime not found, call refused) the lane is a normal-priority torch stream: slower by ~1 %, never wrong."""
    import ctypes
    if priority <= 0:
        return torch.cuda.Stream(device=device, priority=priority)
    rt = _hip_runtime()
    if rt is None:
        return torch.cuda.Stream(device=device, priority=0)
    h = ctypes.c_void_p()
    with torch.cuda.device(device):
        rc = rt.hipStreamCreateWithPriority(ctypes.byref(h), 1, priority)   # 1 = hipStreamNonBlocking
    if rc != 0 or not h.value:
        return torch.cuda.Stream(device=device, priority=0)
    return torch.cuda.ExternalStream(h.value, device=device)


FORK_PRIORITY = int(os.environ.get("SSCG_FORK_PRIORITY", "0"))


def side_priority():
    """Priority of the side lanes (weight gradients, frozen generators, D step): LOW on a single GPU - the dispatcher then prefers
    the critical path's workgroups whenever both are ready (-1.3 ms per config-2 step, same-box A/B) - but NORMAL once a process
    group is up: with RCCL's stream in flight the low-priority lanes cost +30 % (176-190 vs 145 ms, `SSCG_FORCE_DP=1`, measured)."""
    env = os.environ.get("SSCG_SIDE_PRIORITY")
    if env is not None:
        return int(env)
    import torch.distributed as dist
    return 0 if (dist.is_available() and dist.is_initialized()) else 1


def side_priority_for(pixels_per_batch):
    """... and only where the lanes compete for CUs: below ~128 K pixels per batch the kernels do not fill the chip, a low-priority
    lane is merely late at the next join (64x64, batch 2: 48-51 -> 55-61 ms per step)."""
    p = side_priority()
    return p if (p <= 0 or os.environ.get("SSCG_SIDE_PRIORITY") is not None or pixels_per_batch >= 131072) else 0


def set_side_priority(prio):
    """Choose the side lanes' priority - effective only while the process has no lanes yet.  ONE set of lanes per process: a second
    set (a small model at normal priority, then a large one at low priority) oversubscribes the hardware queues - the step ran 172
    instead of 142 ms and produced non-finite losses on this runtime (`tools/nan_probe.sh`, profiles/r03_experiments.txt item 12).
    The first model that steps decides; returns the priority in force."""
    if not SideStream._streams:
        SideStream.priority = prio
    return SideStream.priority


def reset_side_streams():
    """Drop the cached side lanes (they are re-created, with the priority that holds now, on their next use)."""
    if SideStream._streams:
        flush_side_work()
        torch.cuda.synchronize()
        SideStream._streams.clear()
        _STREAM_BY_HANDLE.clear()
    SideStream.priority = None


class SideStream:
    """A second HIP stream per device for work that is independent of the main stream's critical path:
    weight gradients (needed only by the optimiser step) and the frozen generators' forward (needed only by
    the discriminator step).  Two kernels in flight let the dispatcher fill the CUs that one launch with an
    awkward workgroup count (8712-row DeepLab maps: 548 workgroups on 256 CUs) leaves idle."""

    enabled = True
    _streams = {}

    # A/B aid only: with a third lane (or a second lane set) streams share hardware queues, and the overlapped D step then produces
    # non-finite losses (open issue, profiles/r03_experiments.txt items 12-13)
    lanes = int(os.environ.get("SSCG_SIDE_LANES", "2"))   # measured: 4 streams in flight (main, fork lane, 2 side lanes) is the sweet spot; a 5th costs 20 %

    priority = None     # fixed when the first lane is made: set_side_priority() of the first model that steps, else side_priority()

    @classmethod
    def get(cls, device, lane=0):
        s = cls._streams.get((device, lane))
        if s is None:
            if cls.priority is None:
                cls.priority = side_priority()
            s = _make_stream(device, cls.priority)
            cls._streams[(device, lane)] = s
        return s

    @classmethod
    def join(cls, device=None):
        """Make the current stream wait for everything queued on the side stream(s) (deferred work is launched first)."""
        flush_side_work(device)
        for (dev, _), s in cls._streams.items():
            if device is None or dev == device:
                torch.cuda.current_stream(dev).wait_stream(s)


class ForkStream:
    """A third HIP stream: the second lane of the forked generator forwards (model.semisuper_cycleGAN.step).  The
    step's five trainable DeepLab passes form two independent chains, Gis(onehot) -> Gsi(fake_img) and
    Gsi(unl) -> Gis(fake_gt), plus Gsi(l_img); autograd replays each op's backward on the stream of its forward, so
    forking the forward also runs the two backward chains side by side."""

    _streams = {}

    @classmethod
    def get(cls, device, lane=0):
        s = cls._streams.get((device, lane))
        if s is None:
            s = _make_stream(device, FORK_PRIORITY)
            cls._streams[(device, lane)] = s
        return s

    @classmethod
    def join(cls, device):
        for (dev, _), s in cls._streams.items():
            if dev == device:
                torch.cuda.current_stream(device).wait_stream(s)


def lane_events(device):
    """An event on every lane that may carry gradient kernels of the current backward pass - the calling stream, the fork lane, the
    side lanes (deferred side-lane work is launched first): a stream that waits for all of them sees every gradient kernel queued
    so far (parallel.GradBuckets orders a bucket's all-reduce behind them)."""
    flush_side_work(device)
    streams = [torch.cuda.current_stream(device)]
    for reg in (ForkStream._streams, SideStream._streams):
        for (dev, _), st in reg.items():
            if dev == device:
                streams.append(st)
    evs = []
    for st in streams:
        ev = torch.cuda.Event()
        ev.record(st)
        evs.append(ev)
    return evs


# Data parallelism with bucketed gradient exchange (parallel.GradBuckets): GRAD_READY[0] is called with a parameter once the LAST
# gradient kernel of this backward pass that accumulates into its arena slice has been queued.  "Last" is known by counting: the
# forward of a conv node whose weight will receive a gradient counts one use of its weight and bias and keeps them on ctx
# (ctx.counted = _note_use(w, bias)); the node's backward takes back exactly those (_note_done(ctx.counted)) once their gradient
# kernels are queued.  "Will receive a gradient" = ctx.needs_input_grad AND the grad mode of the node's caller, which the wrappers
# below pass into apply() (inside forward() it is always off): needs_input_grad is True for a trainable weight under torch.no_grad()
# as well, but such a forward never sees a backward - it must neither count a use nor keep pre-norm activations alive for one (the
# unused Gis(lab_gt) pass of a step, evaluation, validation).
GRAD_READY = [None]


def _note_use(*params):
    """Counts one use of each parameter that takes part in the exchange; returns the parameters counted."""
    if GRAD_READY[0] is None:
        return ()
    counted = tuple(p for p in params if p is not None and getattr(p, "_sscg_grad", None) is not None)
    for p in counted:
        p._sscg_uses = getattr(p, "_sscg_uses", 0) + 1
    return counted


def _note_done(counted):
    hook = GRAD_READY[0]
    for p in counted:
        p._sscg_uses -= 1
        if p._sscg_uses == 0 and hook is not None:
            hook(p)


def d_stream(device):
    """Stream of the overlapped discriminator step: the LAST side lane - idle between the end of a backward pass and
    the next one, which is when the D step runs.  Not a stream of its own: a fifth stream in flight costs ~20 % (the
    hardware runs four queues side by side; more are time-sliced)."""
    return SideStream.get(device, SideStream.lanes - 1)


def debug_wait_for_d(device, names):
    """Bisection aid (SSCG_DBG_TOPWAIT=main,fork,side0,...): order the named streams behind the D stream."""
    d = d_stream(device)
    for n in names:
        if n == "main":
            s = torch.cuda.current_stream(device)
        elif n == "fork":
            s = ForkStream.get(device)
        else:
            s = SideStream.get(device, int(n[4:]))
        if s.cuda_stream != d.cuda_stream:
            s.wait_stream(d)


def run_on_side_stream(device, tensors, fn, lane=0, defer=False):
    """Launch `fn`'s kernels on the side stream after everything queued so far on the current stream.
    `tensors` are the buffers fn reads: the allocator must not recycle them before the side stream is done.

    defer=True (weight / bias gradient kernels: nothing reads their result before SideStream.join): the call is queued per lane
    and launched in batches of SIDE_BATCH - one stream switch (current_stream + wait_stream + stream guard + record_stream:
    ~20 us of host time) per batch instead of per convolution; 440 switches per step were the largest single item of the
    backward's issue cost.  A parameter's gradient kernels keep their order (FIFO on their own lane)."""
    if not SideStream.enabled:
        return fn()
    lane %= SideStream.lanes
    if defer and SIDE_BATCH[0] > 1:
        q = _SIDE_PENDING.setdefault((device, lane), [])
        q.append((fn, tensors, _stream()))
        if len(q) >= SIDE_BATCH[0]:
            _flush_lane(device, lane)
        return None
    main = torch.cuda.current_stream(device)
    side = SideStream.get(device, lane)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        r = fn()
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    return r


# (8 until the end of round 6; re-swept on the final kernels, profiles/r06_experiments.txt item 27: 4 / 8 / 16 alike, 32 -0.45 and
# -0.8 ms per config-2 step on two boxes, 64 +0.4; config 3 indifferent)
SIDE_BATCH = [int(os.environ.get("SSCG_SIDE_BATCH", "32"))]
_SIDE_PENDING = {}      # (device, lane) -> [(fn, tensors, raw handle of the stream that produced the tensors)]
_STREAM_BY_HANDLE = {}  # raw stream handle -> torch.cuda.Stream (built once per stream: the object costs ~6 us to make)


def _stream_object(device, handle):
    so = _STREAM_BY_HANDLE.get((device, handle))
    if so is None:
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream == handle:
            so = cur
        else:       # a producer stream that is not current any more: every stream this package creates is in the two registries
            for reg in (SideStream._streams, ForkStream._streams):
                for key, st in reg.items():
                    if key[0] == device and st.cuda_stream == handle:
                        so = st
            if so is None:
                so = torch.cuda.ExternalStream(handle, device=device)
        _STREAM_BY_HANDLE[(device, handle)] = so
    return so


def _flush_lane(device, lane):
    q = _SIDE_PENDING.get((device, lane))
    if not q:
        return
    _SIDE_PENDING[(device, lane)] = []
    side = SideStream.get(device, lane)
    for h in {h for _, _, h in q}:
        if h != side.cuda_stream:
            side.wait_stream(_stream_object(device, h))      # behind everything its producers have queued so far
    with torch.cuda.stream(side):
        for fn, _, _ in q:
            fn()
    for _, tensors, _ in q:
        for t in tensors:
            if t is not None:
                t.record_stream(side)


def flush_side_work(device=None):
    """Launch every deferred side-lane call (SideStream.join does this first)."""
    for (dev, lane) in list(_SIDE_PENDING.keys()):
        if device is None or dev == device:
            _flush_lane(dev, lane)


def empty_nhwc(n, c, h, w, device, dtype=torch.float32):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=CL)


def to_nhwc(x):
    """Logical NCHW tensor -> channels-last memory (HIP transpose kernel when a copy is needed)."""
    _need_hip(x)
    if x.dim() != 4:
        raise _lib.SscgError("4-D tensor expected")
    if x.is_contiguous(memory_format=CL):
        return x
    _need_hip(x, f32_only=True)      # bf16 tensors only exist inside the networks, where every kernel writes channels-last
    if not x.is_contiguous():
        x = x.contiguous()
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, h, w, x.device)
    check(lib.sscg_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), n, c, h, w, _stream()), "sscg_nchw_to_nhwc")
    return y


def to_nchw(x):
    """channels-last tensor -> standard contiguous NCHW memory."""
    if x.dtype == torch.bfloat16:
        x = cast(x, torch.float32)
    _need_hip(x)
    if x.is_contiguous():
        return x
    x = to_nhwc(x)
    n, c, h, w = x.shape
    y = torch.empty((n, c, h, w), dtype=x.dtype, device=x.device)
    check(lib.sscg_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), n, c, h, w, _stream()), "sscg_nhwc_to_nchw")
    return y


# What `--dtype f32` computes its contractions with: False = exact fp32 MFMA (v_mfma_f32_32x32x2_f32), True = the fp32-accurate split
# contraction on the bf16 matrix cores (conv_split.hip) wherever the library offers it.
F32_SPLIT = [os.environ.get("SSCG_F32_SPLIT", "1") == "1"]
_MODE = ["f32s" if F32_SPLIT[0] else "f32"]
FUSE_STATS = [os.environ.get("SSCG_FUSE_STATS", "1") != "0"]    # norm statistics from the producing conv's epilogue (K3/K4)
# The reduction pass of a norm layer's backward from the epilogue of the data gradient that produces its upstream gradient
# (sscg_conv2d_dgrad_bsums): ~260 col_reduce launches fewer per step.  fp32 tensors: ON - the split kernel takes
# the sums in its coalesced store phase (config 2 134.4 -> 134.0 ms, host issue time -2 ms per step; the first version, sums in the
# MFMA layout, LOST 0.7 ms).  bf16 tensors: ON since round 6 - rounds 4-5 took them in conv16_kernel's MFMA layout (per-element
# 2-byte gathers of the layer's input: config 3 +1.9 ... +3 ms) and a first store-phase version lost too (64 -> 111 VGPRs); the round-6
# store phase (16-byte row segments requested with the addend's, fp32 over a thread's rows, shuffles across a wave's row lanes,
# fp64 across the waves, one record per tile; its own instances, 128 VGPRs without the fan-in code) wins 1.05 ms at config 3
# (profiles/r06_experiments.txt item 17).  SSCG_FUSE_BSUMS=1 / 0 forces both on / off, "f32" = fp32 tensors only.
_FB = os.environ.get("SSCG_FUSE_BSUMS", "1")
FUSE_BSUMS = [_FB != "0"]            # master switch (tests flip it)
FUSE_BSUMS_BF16 = [_FB == "1"]
# A data gradient that takes the backward sums of a ReLU unit has that unit's mask in registers: it stores the MASKED gradient
# (sscg_conv2d_dgrad_bsums_masked), and the unit's apply pass reads neither the mask source again nor writes the residual's gradient -
# that is the masked gradient itself, the same tensor.  fp32 tensors, ReLU only: where the records are not honoured after all (autograd
# accumulated into the tensor) the ordinary pass masks a second time, which a 0 / 1 mask allows bit for bit and LeakyReLU's does not.
PREMASK = [os.environ.get("SSCG_PREMASK", "1") != "0"]          # (tests flip it)


def set_conv_precision(mode):
    """Arithmetic of the networks (host-side policy; the library itself keeps no mode - every call carries its dtypes):
      "f32"   (default, the reference's dtype, BASELINE config 2): fp32 tensors.  Which contraction that means is the build-wide
              policy F32_SPLIT (env SSCG_F32_SPLIT, default on): "f32s" below, or "f32x";
      "f32s"  fp32 tensors; forward / data-gradient contractions of every conv with >= 32 source channels (a multiple of 32) run as
              the fp32-accurate split contraction on the BF16 matrix cores (conv_split.hip: each operand as three bfloat16 pieces,
              six exact piece products accumulated in fp32; the weights' pieces are kept by the Adam kernel / the operand-copy
              cache, the activations are split between LDS and the matrix cores); weight gradients, few-channel stems and heads
              run the exact fp32 MFMA kernels;
      "f32x"  fp32 tensors, exact fp32 MFMA contractions everywhere (v_mfma_f32_32x32x2_f32);
      "bf16"  (BASELINE configs 3/5): activations and conv-weight operand copies are bfloat16 in HBM, bf16 LDS tiles,
              v_mfma_f32_32x32x16_bf16 with fp32 accumulation; network inputs/outputs, norm statistics, losses, weight
              gradients, master weights and Adam moments stay fp32;
      "bf16c" (round-1 mode): fp32 tensors, operands rounded to bf16 between LDS and the matrix cores."""
    m = {"f32": "f32", "fp32": "f32", "float32": "f32", "bf16": "bf16", "bfloat16": "bf16", "bf16c": "bf16c", "f32s": "f32s",
         "f32x": "f32x"}.get(str(mode).lower())
    if m is None:
        raise _lib.SscgError("conv precision must be 'f32', 'f32x', 'f32s', 'bf16' or 'bf16c', got %r" % (mode,))
    if m == "f32":          # fp32 tensors: which contraction "f32" means is a build-wide policy (F32_SPLIT); "f32x" / "f32s" name one
        m = "f32s" if F32_SPLIT[0] else "f32"
    elif m == "f32x":
        m = "f32"
    if m != _MODE[0]:
        # which operand copies (transposed fp32 / bf16 / split planes) a weight needs depends on the mode: forget the old mode's
        # registrations, or every later step keeps rebuilding copies nothing reads
        for _, kinds in globals().get("_WT_USERS", {}).values():
            kinds.clear()
    _MODE[0] = m


def get_conv_precision():
    return _MODE[0]


if os.environ.get("SSCG_CONV_PRECISION"):          # tools/ and ad-hoc runs; main.py / bench.py take --dtype
    set_conv_precision(os.environ["SSCG_CONV_PRECISION"])


def cast(x, dtype):
    """dtype conversion on the device (fp32 <-> bf16, RNE); layout (strides) preserved."""
    _need_hip(x)
    if x.dtype == dtype:
        return x
    if not (x.is_contiguous() or x.is_contiguous(memory_format=CL)):
        x = x.contiguous()
    y = torch.empty_like(x, dtype=dtype, memory_format=torch.preserve_format)
    check(lib.sscg_cast(x.data_ptr(), _dt(x), y.data_ptr(), _DT[dtype], x.numel(), _stream()), "sscg_cast")
    return y


def conv_out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


_DESC_CACHE = {}


TUNING = [int(os.environ.get("SSCG_TUNING", "0"), 0)]        # sscg_conv_desc.tuning of every descriptor built from here on (tools/ and tile-class tests; 0 = the library's plan)
WGRAD_TUNING = [int(os.environ.get("SSCG_WGRAD_TUNING", "0"), 0)]  # sscg_conv_desc.wgrad_tuning, likewise (env: A/B aid)


def tuning(tile_class=None, split=0, wgrad_class=None, wgrad_splits=0, wgrad_flags=0):
    """Set the per-call tuning fields of the descriptors built from here on (None / 0 = the library's own plans).  Returns the
    previous pair: `old = F.tuning(tile_class=1); ...; F.TUNING[0], F.WGRAD_TUNING[0] = old`."""
    old = (TUNING[0], WGRAD_TUNING[0])
    TUNING[0] = (0 if tile_class is None else tile_class + 1) | (split << 8)
    WGRAD_TUNING[0] = (0 if wgrad_class is None else wgrad_class + 1) | (wgrad_splits << 8) | (wgrad_flags << 24)
    return old


def make_desc(xshape, wshape, stride, pad, dil, pad_mode=PAD_ZEROS, act=ACT_NONE, slope=0.0, xdt=F32, wdt=F32, ydt=F32, prec=0, wplane=0):
    """ConvDesc of a call, memoised (a step re-issues the same few dozen geometries thousands of times, and the host side
    of a launch is what bounds the 4-stream schedule)."""
    key = (tuple(xshape), tuple(wshape), stride, pad, dil, pad_mode, act, slope, xdt, wdt, ydt, prec, TUNING[0], WGRAD_TUNING[0], wplane)
    d = _DESC_CACHE.get(key)
    if d is None:
        d = _DESC_CACHE[key] = _build_desc(xshape, wshape, stride, pad, dil, pad_mode, act, slope)
        d.x_dtype, d.w_dtype, d.y_dtype, d.precision = xdt, wdt, ydt, prec
        d.tuning, d.w_plane, d.wgrad_tuning = TUNING[0], wplane, WGRAD_TUNING[0]
    return d


_SPLIT_OK = {}


def split_applies(xshape, wshape, stride, pad, dil, pad_mode, kind):
    """Does the library's split contraction (fp32 accuracy on the bf16 matrix cores) serve this product?  kind: 0 forward,
    1 data gradient, 2 weight gradient.  The library decides (sscg_conv2d_split_applies); the answer is cached per geometry."""
    key = (tuple(xshape), tuple(wshape), stride, pad, dil, pad_mode, kind)
    v = _SPLIT_OK.get(key)
    if v is None:
        d = _build_desc(xshape, wshape, stride, pad, dil, pad_mode, ACT_NONE, 0.0)
        v = _SPLIT_OK[key] = bool(lib.sscg_conv2d_split_applies(C.byref(d), kind))
    return v


# Products the split mode covers (bisection aid).  The weight gradient has no pre-split operand: BOTH of its operands are split
# between LDS and the matrix cores, which makes the kernel VALU-bound and no faster than the exact fp32 one when it runs alone -
# but it then needs 2.7x fewer matrix-core cycles, and in the step's four-stream schedule those go to the forward / data-gradient
# kernels running beside it: 156.6 -> 148.7 ms per step (SSCG_WGRAD_SPLIT=0 restores the exact fp32 weight gradient).
SPLIT_KINDS = {"fwd", "dgrad"} | ({"wgrad"} if os.environ.get("SSCG_WGRAD_SPLIT", "1") == "1" else set())


def _prec(kind="fwd"):
    """`precision` field for fp32-tensor contractions: 1 = bf16 rounding between LDS and the matrix cores (both bf16 modes); the
    split mode selects its kernels through the weight operand's dtype (SSCG_BF16X3), not through this field."""
    if _MODE[0] == "f32s" and kind == "wgrad" and "wgrad" in SPLIT_KINDS:
        return 2
    return 0 if _MODE[0] in ("f32", "f32s") else 1


_PLAN_SIZES = {}


def _ws_bytes(d, which):
    """Workspace size of a conv entry point.  The split plans depend on the geometry and on the descriptor's tuning fields: cached
    per (descriptor object - one per geometry / dtype / tuning, make_desc - , entry point)."""
    key = (id(d), which)
    v = _PLAN_SIZES.get(key)
    if v is None:
        v = _PLAN_SIZES[key] = getattr(lib, "sscg_conv2d_%s_workspace" % which)(C.byref(d))
    return v


def _stats_bytes(d, g, l):
    key = (id(d), "stats", g, l)
    v = _PLAN_SIZES.get(key)
    if v is None:
        v = _PLAN_SIZES[key] = lib.sscg_conv2d_fwd_stats_bytes(C.byref(d), g, l)
    return v


def _build_desc(xshape, wshape, stride, pad, dil, pad_mode, act, slope):
    n, c, h, w = xshape
    k, c2, r, s = wshape
    if c != c2:
        raise _lib.SscgError("conv channel mismatch: input %d vs weight %d" % (c, c2))
    d = ConvDesc()
    d.N, d.H, d.W, d.C = n, h, w, c
    d.K, d.R, d.S = k, r, s
    d.P, d.Q = conv_out_size(h, r, stride, pad, dil), conv_out_size(w, s, stride, pad, dil)
    d.stride, d.pad, d.dil = stride, pad, dil
    d.pad_mode, d.act, d.slope = pad_mode, act, slope
    return d


# ----------------------------------------------------------------------------- per-kernel timing hook (bench.py)
class ConvProfile:
    """Collects (kind, algorithmic flops, HIP-event pair) for every conv launch while active.  Events are
    recorded on torch's current stream - the stream the kernels are launched on."""

    active = None

    def __init__(self):
        self.records = []

    def __enter__(self):
        ConvProfile.active = self
        return self

    def __exit__(self, *a):
        ConvProfile.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, flops, key, e0, e1, nbytes in self.records:      # kind = (fwd|dgrad|wgrad, kernel family f32|bf16)
            s = out.setdefault(kind, {"launches": 0, "flops": 0.0, "ms": 0.0, "bytes": 0.0, "shapes": {}})
            ms = e0.elapsed_time(e1)
            s["launches"] += 1
            s["flops"] += flops
            s["bytes"] += nbytes
            s["ms"] += ms
            sh = s["shapes"].setdefault(key, [0, 0.0, 0.0])
            sh[0] += 1
            sh[1] += flops
            sh[2] += ms
        return out


def _unprofiled(fn):
    prof, ConvProfile.active = ConvProfile.active, None
    try:
        return fn()
    finally:
        ConvProfile.active = prof


def _timed(kind, d, fn, extra_bytes=0):
    """extra_bytes: algorithmic reads of a launch's fused store phase beyond operands and result (the fan-in addend, the normalisation
    layer's input and mask source of a data gradient that takes the backward sums)."""
    prof = ConvProfile.active
    if prof is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    flops = 2.0 * d.N * d.P * d.Q * d.K * d.R * d.S * d.C
    key = "%dx%dx%d c%d k%d r%d s%d p%d d%d" % (d.N, d.H, d.W, d.C, d.K, d.R, d.stride, d.pad, d.dil)
    # which kernel family the library dispatches to (include/sscg.h, "Supported dtype combinations")
    if kind == "fwd":
        b16 = d.x_dtype == BF16 and d.w_dtype == BF16
    elif kind == "dgrad":
        b16 = d.y_dtype == BF16 and d.w_dtype == BF16
    else:
        b16 = d.x_dtype == BF16 and d.y_dtype == BF16 and d.K >= 32 and d.R * d.S * d.C >= 32
    # algorithmic HBM bytes of the launch: every operand read once, the result written once
    esz = {F32: 4, BF16: 2, BF16X3: 6}
    nbytes = (d.N * d.H * d.W * d.C * esz[d.x_dtype] + d.N * d.P * d.Q * d.K * esz[d.y_dtype]
              + d.K * d.R * d.S * d.C * (4 if kind == "wgrad" else esz[d.w_dtype])) + extra_bytes
    prof.records.append(((kind, "split" if d.w_dtype == BF16X3 else ("bf16" if b16 else "f32")), flops, key, e0, e1, float(nbytes)))
    return r


# ----------------------------------------------------------------------------- raw ops
def _fwd_operands(x, w, geom=None):
    """(weight operand, its dtype code, plane stride) for a forward whose input is x: bf16 tiles when x is a bf16 activation
    with a multiple of 64 channels; the three-plane split copy in the split mode where the library's split kernels serve the
    geometry `geom` = (stride, pad, dil, pad_mode); else the fp32 kernel on the fp32 master weight (stems, few-channel inputs)."""
    if x.dtype == torch.bfloat16:
        if x.shape[1] % 64:
            raise _lib.SscgError("bf16 activations with %d channels: the bf16 conv kernels need a multiple of 64" % x.shape[1])
        return weight_bf16(w), BF16, 0
    if _MODE[0] == "f32s" and "fwd" in SPLIT_KINDS and geom is not None and split_applies(x.shape, w.shape, *geom, 0):
        ws, plane = weight_split(w)
        return ws, BF16X3, plane
    return w, F32, 0


def _out_dtype(out_f32):
    return torch.bfloat16 if (_MODE[0] == "bf16" and not out_f32) else torch.float32


PAD_STEMS = [os.environ.get("SSCG_PAD_STEMS", "1") != "0"]


def resize_channels(x, c_new):
    """[N, C, H, W] (channels-last) or a [K, C, R, S] weight -> the same with c_new channels: zero-padded or cut (fp32)."""
    x = x if x.is_contiguous(memory_format=CL) else x.contiguous(memory_format=CL)
    n, c, h, w = x.shape
    y = empty_nhwc(n, c_new, h, w, x.device)
    check(lib.sscg_resize_channels(x.data_ptr(), y.data_ptr(), n * h * w, c, c_new, _stream()), "sscg_resize_channels")
    return y


def _padded_stem(xshape, wshape, stride, pad, dil, pad_mode, kind):
    """Split mode: a convolution over 17-31 source channels (the 21 / 20-channel stems on one-hot / softmax maps: arch/generators.py:73,
    373) runs as a 32-channel convolution on the split contraction - the extra channels are zero in the activation AND in the weight
    copy - instead of the exact-fp32 kernel's ragged-channel path (57 TFLOP/s): returns 32 when the padded geometry is served."""
    c = xshape[1]
    if not (PAD_STEMS[0] and _MODE[0] == "f32s" and 16 < c < 32 and wshape[0] >= 16):
        return 0
    kname = "fwd" if kind == 0 else "dgrad"
    if kname not in SPLIT_KINDS:
        return 0
    xs = (xshape[0], 32, xshape[2], xshape[3])
    ws = (wshape[0], 32, wshape[2], wshape[3])
    return 32 if split_applies(xs, ws, stride, pad, dil, pad_mode if kind == 0 else PAD_ZEROS, kind) else 0


def _padded_head(xshape, wshape, stride, pad, dil):
    """Split mode: the data gradient of a convolution with 17-31 OUTPUT channels (the reduction runs over taps x output channels: 21
    is no multiple of the 32-wide k-tile) runs with dy and the filters padded to 32 output channels: returns 32 when served."""
    k = wshape[0]
    if not (PAD_STEMS[0] and _MODE[0] == "f32s" and 16 < k < 32 and "dgrad" in SPLIT_KINDS):
        return 0
    return 32 if split_applies(xshape, (32,) + tuple(wshape[1:]), stride, pad, dil, PAD_ZEROS, 1) else 0


def _pad_filters(w, k_new):
    """[K, C, R, S] -> [k_new, C, R, S] with zero filters appended (a device copy of the K * R * S * C leading elements)."""
    w = w if w.is_contiguous(memory_format=CL) else w.contiguous(memory_format=CL)
    wp = empty_nhwc(k_new, w.shape[1], w.shape[2], w.shape[3], w.device)
    fill_(wp, 0.0)
    wp[:w.shape[0]].copy_(w)
    return wp


def _padded_weight(w, c_new):
    """The weight with zero-padded source channels, cached on the weight (rebuilt when the optimiser rewrites it); its own operand
    copies (split planes, transposed split planes) are cached on the padded tensor and die with it."""
    return _cached_copy(w, "_sscg_wpad", lambda: resize_channels(w.detach(), c_new))


def conv2d_fwd(x, w, bias, stride=1, pad=0, dil=1, pad_mode=PAD_ZEROS, act=ACT_NONE, slope=0.0, out_f32=True, stats=None):
    """y = act(conv(x, w) + bias).  out_f32: keep the output fp32 in bf16 mode (network heads).
    stats = (G, L): also return the epilogue's column statistics buffer (None when the fusion does not apply)."""
    if act == ACT_TANH and w.shape[0] > 32 and x.dtype == torch.bfloat16:
        # (no such layer in the reference's nets: the bf16 kernels carry tanh in their 32-column heads' class only)
        return act_fwd(conv2d_fwd(x, w, bias, stride, pad, dil, pad_mode, ACT_NONE, 0.0, out_f32), ACT_TANH, 0.0)
    if x.dtype == torch.float32:
        cp = _padded_stem(x.shape, w.shape, stride, pad, dil, pad_mode, 0)
        if cp:
            # (the profile books this launch - padding pass included - under the ORIGINAL geometry: algorithmic FLOP of the 21-channel conv)
            d0 = make_desc(x.shape, w.shape, stride, pad, dil, pad_mode, act, slope, F32, BF16X3, F32, _prec(), 0)
            return _timed("fwd", d0, lambda: _unprofiled(lambda: conv2d_fwd(resize_channels(x, cp), _padded_weight(w, cp), bias, stride, pad, dil,
                                                                             pad_mode, act, slope, out_f32, stats)))
    # (a fused tanh behind more than 32 output channels - no such layer in the reference's nets - stays on the exact kernel: the split
    # family's epilogue carries tanh in its heads' class only)
    wop, wdt, wplane = _fwd_operands(x, w, None if (act == ACT_TANH and w.shape[0] > 32) else (stride, pad, dil, pad_mode))
    ydt = _out_dtype(out_f32)
    d = make_desc(x.shape, w.shape, stride, pad, dil, pad_mode, act, slope, _dt(x), wdt, _DT[ydt], _prec(), wplane)
    y = empty_nhwc(d.N, d.K, d.P, d.Q, x.device, ydt)
    ws = _WS.get(_ws_bytes(d, "fwd"), x.device)
    if stats is not None:
        nb = _stats_bytes(d, int(stats[0]), int(stats[1]))
        if nb:
            sbuf = torch.empty(nb, dtype=torch.uint8, device=x.device)
            _timed("fwd", d, lambda: check(lib.sscg_conv2d_fwd_stats(C.byref(d), x.data_ptr(), wop.data_ptr(), _ptr(bias), y.data_ptr(),
                                                                     int(stats[0]), int(stats[1]), sbuf.data_ptr(), nb, ws.data_ptr(),
                                                                     ws.numel(), _stream()), "sscg_conv2d_fwd_stats"))
            return y, (d, sbuf)
    _timed("fwd", d, lambda: check(lib.sscg_conv2d_fwd(C.byref(d), x.data_ptr(), wop.data_ptr(), _ptr(bias), y.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), _stream()), "sscg_conv2d_fwd"))
    return (y, None) if stats is not None else y


def norm_stats_from_conv(cs, per_sample_glc, eps, running_mean=None, running_var=None, momentum=0.1):
    """mean / rstd (and the running-statistics update) from the statistics a conv epilogue left (conv2d_fwd(..., stats=))."""
    d, sbuf = cs
    g, l, c = per_sample_glc
    mean = torch.empty((g, c), dtype=torch.float32, device=sbuf.device)
    rstd = torch.empty((g, c), dtype=torch.float32, device=sbuf.device)
    check(lib.sscg_norm_stats_from_conv(C.byref(d), sbuf.data_ptr(), g, l, eps, mean.data_ptr(), rstd.data_ptr(), _ptr(running_mean),
                                        _ptr(running_var), momentum, _stream()), "sscg_norm_stats_from_conv")
    return mean, rstd


def conv2d_fwd_norm(x, w, bias, stride, pad, dil, pad_mode, out_f32, glc, eps, running_mean=None, running_var=None, momentum=0.1):
    """(y, mean, rstd): y = conv(x, w) + bias with the batch statistics of the normalisation layer that follows (view [G][L][C] of y;
    running statistics updated): the conv's epilogue takes the statistics, one small launch finalises them.  mean is None when no conv
    epilogue takes statistics for this geometry (the caller runs a statistics pass over y)."""
    g, l, c = glc
    y, cs = conv2d_fwd(x, w, bias, stride, pad, dil, pad_mode, ACT_NONE, 0.0, out_f32, stats=(g, l))
    if cs is None:
        return y, None, None
    mean, rstd = norm_stats_from_conv(cs, glc, eps, running_mean, running_var, momentum)
    return y, mean, rstd


FUSE_FRONT = [os.environ.get("SSCG_FUSE_FRONT", "1") != "0"]      # A/B aid: PixelDiscriminator's two leading convs as separate launches
FRONT_CALLS = [0]                                                  # fused front launches issued (tests assert the path taken)


def conv2d_front_applies(x, w1, w, stride, pad, dil, pad_mode):
    """Does ONE launch serve Conv2d(cin, 64, 1x1) -> LeakyReLU -> Conv2d(64, K, 1x1) (PixelDiscriminator's front half,
    arch/discriminators.py:70-73) on this input?  fp32 tensors in the split mode, cin in {3, 4, 20, 21}; the library decides the rest."""
    if not (FUSE_FRONT[0] and _MODE[0] == "f32s" and "fwd" in SPLIT_KINDS and x.dtype == torch.float32 and x.is_cuda):
        return False
    if not (tuple(w1.shape[2:]) == (1, 1) and tuple(w.shape[2:]) == (1, 1) and w1.shape[0] == w.shape[1] == 64
            and stride == 1 and pad == 0 and dil == 1 and pad_mode == PAD_ZEROS):
        return False
    n, cin, h, wd = x.shape
    key = ("front", n, cin, h, wd, w.shape[0], TUNING[0])
    v = _SPLIT_OK.get(key)
    if v is None:
        ws, plane = None, w.numel()
        d = make_desc((n, 64, h, wd), w.shape, 1, 0, 1, PAD_ZEROS, ACT_NONE, 0.0, F32, BF16X3, F32, _prec(), plane)
        v = _SPLIT_OK[key] = bool(lib.sscg_conv2d_front_applies(C.byref(d), cin))
    return v


def conv2d_front_fwd(x, w1, b1, slope1, w, bias, glc=None, want_h1=False):
    """(y, h1 or None, cs or None): y = conv(lrelu(conv(x, w1) + b1), w) + bias in one launch; h1 (the 64-channel map between the two
    convs) is written only when asked for; glc = (G, L, C): the launch also leaves the statistics records of the norm layer behind
    it (`cs` for norm_stats_from_conv)."""
    x = to_nhwc(x)
    n, cin, h, wd = x.shape
    wop, plane = weight_split(w)
    d = make_desc((n, 64, h, wd), w.shape, 1, 0, 1, PAD_ZEROS, ACT_NONE, 0.0, F32, BF16X3, F32, _prec(), plane)
    y = empty_nhwc(n, w.shape[0], h, wd, x.device, torch.float32)
    h1 = empty_nhwc(n, 64, h, wd, x.device, torch.float32) if want_h1 else None
    g = l = nb = 0
    sbuf = None
    if glc is not None:
        g, l = int(glc[0]), int(glc[1])
        nb = _stats_bytes(d, g, l)
        if not nb:
            raise _lib.SscgError("conv2d_front_fwd: no fused statistics for this geometry")
        sbuf = torch.empty(nb, dtype=torch.uint8, device=x.device)
    FRONT_CALLS[0] += 1
    w1f = w1.detach().reshape(64, cin)
    if not w1f.is_contiguous():
        w1f = w1f.contiguous()
    # (booked under the second conv's geometry + the front conv's algorithmic FLOP; the bytes are the launch's own: x in, y [+ h1] out)
    _timed("fwd", d, lambda: check(lib.sscg_conv2d_front_fwd(C.byref(d), x.data_ptr(), cin, w1f.data_ptr(), _ptr(b1), float(slope1), _ptr(h1),
                                                             wop.data_ptr(), _ptr(bias), y.data_ptr(), g, l, _ptr(sbuf), nb, _stream()),
                                   "sscg_conv2d_front_fwd"))
    return y, h1, ((d, sbuf) if sbuf is not None else None)


def weight_transposed(w, dtype=torch.float32):
    """[K][R][S][C] -> [C][R][S][K] (the operand layout of sscg_conv2d_dgrad), as fp32 or bf16; dtype "x3" = the three bf16
    planes of the split contraction (a flat bf16 tensor of 3 * numel elements)."""
    k, c, r, s = w.shape
    if dtype == "x3":
        wt = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=w.device)
        check(lib.sscg_weight_krsc_to_crsk(w.data_ptr(), F32, wt.data_ptr(), BF16X3, k, r * s, c, _stream()), "sscg_weight_krsc_to_crsk")
        return wt
    src = w
    if dtype == torch.bfloat16:
        src = weight_bf16(w)            # transposing the bf16 shadow reads half the bytes
    wt = torch.empty((c, k, r, s), dtype=dtype, device=w.device, memory_format=CL)
    check(lib.sscg_weight_krsc_to_crsk(src.data_ptr(), _dt(src), wt.data_ptr(), _DT[dtype], k, r * s, c, _stream()),
          "sscg_weight_krsc_to_crsk")
    return wt


def dgrad_operand(w, xshape, stride, pad, dil, dy_dtype=torch.float32):
    """The transposed operand copy [C][R][S][K] of weight `w` in the form the data gradient of this geometry reads in the current
    mode (uncached: tools and kernel tests; the networks use the per-parameter cache of conv2d_dgrad_param)."""
    if dy_dtype == torch.bfloat16:
        return weight_transposed(w, torch.bfloat16)
    if _MODE[0] == "f32s" and "dgrad" in SPLIT_KINDS and split_applies(xshape, w.shape, stride, pad, dil, PAD_ZEROS, 1):
        return weight_transposed(w, "x3")
    return weight_transposed(w, torch.float32)


def _bsums_bytes(d, g, l):
    key = (id(d), "bsums", g, l)
    v = _PLAN_SIZES.get(key)
    if v is None:
        v = _PLAN_SIZES[key] = lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(d), g, l)
    return v


def _dgrad_add_applies(d):
    key = (id(d), "dgrad_add")
    v = _PLAN_SIZES.get(key)
    if v is None:
        v = _PLAN_SIZES[key] = bool(lib.sscg_conv2d_dgrad_add_applies(C.byref(d)))
    return v


def conv2d_dgrad(dy, wt, xshape, wshape, stride, pad, dil, bias=None, act=ACT_NONE, slope=0.0, out_dtype=torch.float32, bsums=None,
                 addend=None, z=None, premask=False):
    """dx = act(dgrad(dy, wt) + bias); `wt` is the transposed operand copy [C][R][S][K] (weight_transposed), fp32 for an
    fp32 dy, bf16 for a bf16 dy.
    bsums = (nx, mean, rstd, gamma, beta, (G, L, C), act, slope[, residual]): dx is the gradient at the output of
    act(norm(nx) [+ residual]); the launch also takes that layer's backward sums in its epilogue (`residual` true: the mask is read
    off the unit's output `z`, this conv's own input).
    addend: a tensor like dx - the gradient another consumer of the same tensor left - joined in the store phase (dx = dgrad + addend;
    the sums then see the total).
    premask (with bsums of a ReLU unit, fp32 tensors): where the sums are taken, dx is the MASKED gradient - mask ? dgrad + addend : +0,
    what norm_bwd_from_sums would hand back as dres; that call then runs with ACT_NONE and y=None on it.
    With bsums or addend the result is (dx, records, joined): records None where the library does not fuse the geometry (the caller
    runs the ordinary reduction pass; dx is then the unmasked total), joined False where the addend was NOT added (the caller adds)."""
    if act == ACT_TANH and xshape[1] > 32 and dy.dtype == torch.bfloat16 and bsums is None and addend is None:
        return act_fwd(conv2d_dgrad(dy, wt, xshape, wshape, stride, pad, dil, bias, ACT_NONE, 0.0, out_dtype), ACT_TANH, 0.0)
    wdt = BF16X3 if (wt.dim() == 1 and wt.dtype == torch.bfloat16) else _dt(wt)      # the split copy is a flat tensor of three planes
    d = make_desc(xshape, wshape, stride, pad, dil, xdt=_DT[out_dtype], wdt=wdt, ydt=_dt(dy), prec=_prec("dgrad"))
    dx = empty_nhwc(d.N, d.C, d.H, d.W, dy.device, out_dtype)
    ws = _WS.get(_ws_bytes(d, "dgrad"), dy.device)
    want3 = bsums is not None or addend is not None
    plain = bias is None and act == ACT_NONE
    f32 = out_dtype == torch.float32 and dy.dtype == torch.float32
    if addend is not None and not (plain and addend.dtype == out_dtype == dy.dtype and tuple(addend.shape) == tuple(dx.shape)
                                   and addend.stride() == dx.stride() and _dgrad_add_applies(d)):
        addend = None
    joinable = addend is not None
    if joinable and not f32:
        bsums = None            # (bf16 tensors: the addend joins, the sums of a joined gradient are not taken - conv16_kernel)
    if bsums is not None:
        nx, mean, rstd, gamma, beta, (g, l, c), nact, nslope = bsums[:8]
        res = len(bsums) > 8 and bsums[8]
        nb = _bsums_bytes(d, g, l) if (plain and c == d.C and nx.dtype == out_dtype and dy.dtype == out_dtype) else 0
        if res and not (f32 and z is not None and z.dtype == torch.float32 and z.stride() == dx.stride()):
            nb = 0
        if premask and not (nact == ACT_RELU and f32):
            raise _lib.SscgError("conv2d_dgrad: the masked store serves ReLU units on fp32 tensors only")
        if nb:
            entry, name = ((lib.sscg_conv2d_dgrad_bsums_masked, "sscg_conv2d_dgrad_bsums_masked") if premask
                           else (lib.sscg_conv2d_dgrad_bsums, "sscg_conv2d_dgrad_bsums"))
            sums = torch.empty(nb, dtype=torch.uint8, device=dy.device)
            fused_reads = dx.numel() * dx.element_size() * (1 + (1 if res else 0) + (1 if addend is not None else 0))      # nx [, z] [, addend]
            _timed("dgrad", d, lambda: check(entry(
                C.byref(d), dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), nx.data_ptr(), z.data_ptr() if res else None, _ptr(addend),
                mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), g, l, nact, nslope, sums.data_ptr(), nb, ws.data_ptr(),
                ws.numel(), _stream()), name), extra_bytes=fused_reads)
            return dx, (d, sums, res), joinable
    if joinable:
        _timed("dgrad", d, lambda: check(lib.sscg_conv2d_dgrad_add(C.byref(d), dy.data_ptr(), wt.data_ptr(), addend.data_ptr(), dx.data_ptr(),
                                                                   ws.data_ptr(), ws.numel(), _stream()), "sscg_conv2d_dgrad_add"),
               extra_bytes=dx.numel() * dx.element_size())
        return dx, None, True
    _timed("dgrad", d, lambda: check(lib.sscg_conv2d_dgrad(C.byref(d), dy.data_ptr(), wt.data_ptr(), _ptr(bias), dx.data_ptr(),
                                                           act, slope, ws.data_ptr(), ws.numel(), _stream()), "sscg_conv2d_dgrad"))
    return (dx, None, False) if want3 else dx


def conv2d_dgrad_param(dy, w, xshape, wshape, stride, pad, dil, bias=None, act=ACT_NONE, slope=0.0, out_dtype=torch.float32, bsums=None,
                       addend=None, z=None, premask=False):
    """conv2d_dgrad with the transposed operand copy of parameter `w` taken from the per-parameter cache, in the element
    type the kernel for dy reads (bf16 tiles for a bf16 dy, fp32 otherwise)."""
    if dy.dtype == torch.float32 and out_dtype == torch.float32 and bias is None and act == ACT_NONE:
        cp = _padded_stem(xshape, wshape, stride, pad, dil, PAD_ZEROS, 1) if (bsums is None and addend is None) else 0
        if cp:      # the padded weight's data gradient has 32 channels: the extra ones (zero weights: zero gradient) are cut again
            wp = _padded_weight(w, cp)
            xs = (xshape[0], cp, xshape[2], xshape[3])
            d0 = make_desc(xshape, wshape, stride, pad, dil, xdt=F32, wdt=BF16X3, ydt=F32, prec=_prec("dgrad"))
            return _timed("dgrad", d0, lambda: _unprofiled(lambda: resize_channels(
                conv2d_dgrad(dy, _cached_wt(wp, "x3"), xs, tuple(wp.shape), stride, pad, dil), xshape[1])))
        kp = _padded_head(xshape, wshape, stride, pad, dil)
        if kp:      # a 21 / 20-channel head (the DeepLab classifiers): dy and the filters padded to 32 OUTPUT channels - zero gradients
            wp = _cached_copy(w, "_sscg_wpadk", lambda: _pad_filters(w.detach(), kp))       # against zero filters add nothing to dx; the
            d0 = make_desc(xshape, wshape, stride, pad, dil, xdt=F32, wdt=BF16X3, ydt=F32, prec=_prec("dgrad"))      # result has dx's own shape:
            return _timed("dgrad", d0, lambda: _unprofiled(lambda: conv2d_dgrad(      # the fused store phases (fan-in, backward sums) apply
                resize_channels(dy, kp), _cached_wt(wp, "x3"), xshape, tuple(wp.shape), stride, pad, dil, bsums=bsums, addend=addend, z=z,
                premask=premask)))
    if dy.dtype == torch.bfloat16:
        if wshape[0] % 64:
            raise _lib.SscgError("bf16 output gradients with %d channels: the bf16 conv kernels need a multiple of 64" % wshape[0])
        wt = _cached_wt(w, torch.bfloat16)
    elif (_MODE[0] == "f32s" and "dgrad" in SPLIT_KINDS and out_dtype == torch.float32
          and split_applies(xshape, wshape, stride, pad, dil, PAD_ZEROS, 1)):
        wt = _cached_wt(w, "x3")
    else:
        wt = _cached_wt(w, torch.float32)
    return conv2d_dgrad(dy, wt, xshape, wshape, stride, pad, dil, bias, act, slope, out_dtype, bsums, addend, z, premask)


def conv2d_wgrad(x, dy, wshape, stride, pad, dil, pad_mode=PAD_ZEROS, out=None, accumulate=False):
    d = make_desc(x.shape, wshape, stride, pad, dil, pad_mode, xdt=_dt(x), ydt=_dt(dy), prec=_prec("wgrad"))
    if out is None:
        k, c, r, s = wshape
        out = torch.empty((k, c, r, s), dtype=torch.float32, device=x.device, memory_format=CL)
        accumulate = False
    ws = _WS.get(_ws_bytes(d, "wgrad"), x.device)
    _timed("wgrad", d, lambda: check(lib.sscg_conv2d_wgrad(C.byref(d), x.data_ptr(), dy.data_ptr(), out.data_ptr(),
                                                           1.0 if accumulate else 0.0, ws.data_ptr(), ws.numel(), _stream()),
                                     "sscg_conv2d_wgrad"))
    return out


def colsum(x2d_rows, cols, x, out=None, accumulate=False):
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
        accumulate = False
    nb = _cached_size(lib.sscg_colsum_workspace, x2d_rows, cols)
    ws = _WS.get(nb, x.device)
    check(lib.sscg_colsum(x.data_ptr(), _dt(x), out.data_ptr(), x2d_rows, cols, 1.0 if accumulate else 0.0, ws.data_ptr(),
                          ws.numel(), _stream()), "sscg_colsum")
    return out


_SIZE_CACHE = {}


def _cached_size(fn, *args):
    """Workspace size queries that depend on the geometry alone (no tuning hook changes them)."""
    key = (id(fn),) + args
    v = _SIZE_CACHE.get(key)
    if v is None:
        v = _SIZE_CACHE[key] = fn(*args)
    return v


def _glc(x, per_sample):
    return _glc_shape(x.shape, per_sample)


def _glc_shape(shape, per_sample):
    """[G][L][C] view of an NHWC tensor.  per_sample: True = InstanceNorm (G = N), False = BatchNorm (G = 1), an int
    k > 1 = BatchNorm over k batches stacked along N (G = k, each group N/k samples)."""
    n, c, h, w = shape
    if per_sample is True:
        return n, h * w, c
    k = 1 if per_sample is False else int(per_sample)
    if k < 1 or n % k:
        raise _lib.SscgError("batch of %d does not split into %d groups" % (n, k))
    return k, (n // k) * h * w, c


def norm_stats(x, per_sample, eps=1e-5, running_mean=None, running_var=None, momentum=0.1):
    g, l, c = _glc(x, per_sample)
    mean = torch.empty((g, c), dtype=torch.float32, device=x.device)
    rstd = torch.empty((g, c), dtype=torch.float32, device=x.device)
    nb = _cached_size(lib.sscg_norm_stats_workspace, g, l, c)
    ws = _WS.get(nb, x.device)
    check(lib.sscg_norm_stats(x.data_ptr(), _dt(x), g, l, c, eps, mean.data_ptr(), rstd.data_ptr(), _ptr(running_mean),
                              _ptr(running_var), momentum, ws.data_ptr(), ws.numel(), _stream()), "sscg_norm_stats")
    return mean, rstd


def norm_apply(x, mean, rstd, gamma, beta, residual, per_sample, act=ACT_NONE, slope=0.0):
    g, l, c = _glc(x, per_sample)
    y = torch.empty_like(x, memory_format=CL)
    check(lib.sscg_norm_apply(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), _ptr(residual),
                              y.data_ptr(), _same_dtype(x, residual), g, l, c, act, slope, _stream()), "sscg_norm_apply")
    return y


def norm_bwd(dy, x, y, mean, rstd, gamma, per_sample, act, slope, stats_grad=True, want_dres=False, dgamma=None,
             dbeta=None, beta=None, overwrite=False):
    """y None (ReLU / LeakyReLU, no residual in the forward): the activation mask is recomputed from x, gamma, beta."""
    g, l, c = _glc(x, per_sample)
    dx = torch.empty_like(x, memory_format=CL)
    dres = torch.empty_like(x, memory_format=CL) if want_dres else None
    nb = _cached_size(lib.sscg_norm_bwd_workspace, g, l, c)
    ws = _WS.get(nb, x.device)
    check(lib.sscg_norm_bwd(dy.data_ptr(), x.data_ptr(), _ptr(y), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta),
                            dx.data_ptr(), _ptr(dres), _ptr(dgamma), _ptr(dbeta), _same_dtype(x, dy, y), g, l, c, act, slope,
                            (1 if stats_grad else 0) | (2 if overwrite else 0), ws.data_ptr(), ws.numel(), _stream()), "sscg_norm_bwd")
    return dx, dres


def norm_bwd_from_sums(rec, dy, x, mean, rstd, gamma, beta, per_sample, act, slope, dgamma=None, dbeta=None, y=None, want_dres=False):
    """norm_bwd (batch statistics, gradients of gamma / beta written) for a dy whose backward sums the data gradient that produced it
    already took (conv2d_dgrad(..., bsums=)): finalize + apply.  The mask is recomputed from x, or read off the unit's forward output
    y when a residual joined it (want_dres: its gradient, the masked dy).  Returns (dx, dres)."""
    d, sums = rec[0], rec[1]
    g, l, c = _glc(x, per_sample)
    dx = torch.empty_like(x, memory_format=CL)
    dres = torch.empty_like(x, memory_format=CL) if want_dres else None
    ws = _WS.get(g * c * 8, x.device)
    check(lib.sscg_norm_bwd_from_sums(C.byref(d), sums.data_ptr(), dy.data_ptr(), x.data_ptr(), _ptr(y), mean.data_ptr(), rstd.data_ptr(),
                                      _ptr(gamma), _ptr(beta), dx.data_ptr(), _ptr(dres), _ptr(dgamma), _ptr(dbeta), _same_dtype(x, dy), g, l,
                                      c, act, slope, 2, ws.data_ptr(), ws.numel(), _stream()), "sscg_norm_bwd_from_sums")
    return dx, dres


def norm_head_applies(c):
    """Does the one-pass norm -> activation -> 1x1 single-channel conv (PixelDiscriminator's tail) serve a C-channel map?"""
    return bool(lib.sscg_norm_head_applies(int(c)))


def norm_head_fwd(x, mean, rstd, gamma, beta, w, bias, per_sample, act, slope):
    """out[N,1,H,W] (fp32) = bias + sum_c w[c] * act(norm(x)) - one pass over x, the normalised map is never written."""
    g, l, c = _glc(x, per_sample)
    n, _, h, wd = x.shape
    out = torch.empty((n, 1, h, wd), dtype=torch.float32, device=x.device)
    check(lib.sscg_norm_head_fwd(x.data_ptr(), _dt(x), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), w.data_ptr(),
                                 _ptr(bias), out.data_ptr(), g, l, c, act, slope, _stream()), "sscg_norm_head_fwd")
    return out


def norm_head_bwd(dout, w, x, mean, rstd, gamma, beta, per_sample, act, slope, stats_grad, dwb, dgamma=None, dbeta=None):
    """Backward of norm_head_fwd: the gradient at x; dwb[:C] / dwb[C] (written) = the head's weight / bias gradient."""
    g, l, c = _glc(x, per_sample)
    dx = torch.empty_like(x, memory_format=CL)
    nb = _cached_size(lib.sscg_norm_head_bwd_workspace, g, l, c)
    ws = _WS.get(nb, x.device)
    check(lib.sscg_norm_head_bwd(dout.data_ptr(), w.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta),
                                 dx.data_ptr(), dwb.data_ptr(), dwb.data_ptr() + 4 * c, _ptr(dgamma), _ptr(dbeta), _dt(x), g, l, c, act,
                                 slope, (1 if stats_grad else 0) | 2 | 4, ws.data_ptr(), ws.numel(), _stream()), "sscg_norm_head_bwd")
    return dx


def rstd_from_var(var, eps):
    out = torch.empty_like(var)
    check(lib.sscg_rstd_from_var(var.data_ptr(), out.data_ptr(), var.numel(), eps, _stream()), "sscg_rstd_from_var")
    return out


def act_fwd(x, act, slope=0.0):
    y = torch.empty_like(x, memory_format=torch.preserve_format)
    check(lib.sscg_act_fwd(x.data_ptr(), y.data_ptr(), _dt(x), x.numel(), act, slope, _stream()), "sscg_act_fwd")
    return y


def act_bwd(dy, y, act, slope=0.0):
    dx = torch.empty_like(y, memory_format=torch.preserve_format)
    check(lib.sscg_act_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), _same_dtype(y, dy), y.numel(), act, slope, _stream()), "sscg_act_bwd")
    return dx


def add(a, b):
    y = torch.empty_like(a, memory_format=torch.preserve_format)
    check(lib.sscg_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), _same_dtype(a, b), a.numel(), _stream()), "sscg_add")
    return y


def fill_(x, v):
    if x.dtype != torch.float32:
        if v != 0.0 or (x.numel() * x.element_size()) % 4:
            raise _lib.SscgError("fill_ of a %s tensor supports zero only" % x.dtype)
        check(lib.sscg_fill(x.data_ptr(), x.numel() * x.element_size() // 4, 0.0, _stream()), "sscg_fill")
        return x
    check(lib.sscg_fill(x.data_ptr(), x.numel(), float(v), _stream()), "sscg_fill")
    return x


def dropout(x, p, seed):
    y = torch.empty_like(x, memory_format=torch.preserve_format)
    check(lib.sscg_dropout(x.data_ptr(), y.data_ptr(), _dt(x), x.numel(), p, seed, _stream()), "sscg_dropout")
    return y


def gauss_noise(x, sigma, seed):
    """utils.GaussianNoise.forward on the device: x + sigma * x * N(0, 1) (utils.py:133-139)."""
    _need_hip(x, f32_only=True)
    y = torch.empty_like(x, memory_format=torch.preserve_format)
    check(lib.sscg_gauss_noise(x.data_ptr(), y.data_ptr(), x.numel(), float(sigma), int(seed), _stream()), "sscg_gauss_noise")
    return y


def pool_out_size(h):
    """MaxPool2d(3, 2, 1, ceil_mode=True) output size (torch rule: last window must start inside input+left pad)."""
    o = -((-(h + 2 - 3)) // 2) + 1
    if (o - 1) * 2 >= h + 1:
        o -= 1
    return o


def maxpool_fwd(x):
    n, c, h, w = x.shape
    p, q = pool_out_size(h), pool_out_size(w)
    y = empty_nhwc(n, c, p, q, x.device, x.dtype)
    idx = torch.empty((n, c, p, q), dtype=torch.uint8, device=x.device, memory_format=CL)
    check(lib.sscg_maxpool3x3s2_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), _dt(x), n, h, w, c, p, q, _stream()),
          "sscg_maxpool3x3s2_fwd")
    return y, idx


def maxpool_bwd(dy, idx, xshape):
    n, c, h, w = xshape
    p, q = dy.shape[2], dy.shape[3]
    dx = empty_nhwc(n, c, h, w, dy.device, dy.dtype)
    check(lib.sscg_maxpool3x3s2_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), _dt(dy), n, h, w, c, p, q, _stream()),
          "sscg_maxpool3x3s2_bwd")
    return dx


def upsample_fwd(x, oh, ow):
    _need_hip(x, f32_only=True)          # the resize sits on the fp32 side of a network head (model.py:390-392)
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, oh, ow, x.device)
    check(lib.sscg_upsample_bilinear_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow, _stream()), "sscg_upsample_bilinear_fwd")
    return y


def upsample_bwd(dy, h, w):
    n, c, oh, ow = dy.shape
    dx = empty_nhwc(n, c, h, w, dy.device)
    check(lib.sscg_upsample_bilinear_bwd(dy.data_ptr(), dx.data_ptr(), n, h, w, c, oh, ow, _stream()), "sscg_upsample_bilinear_bwd")
    return dx


def reflect_pad(x, pad):
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, h + 2 * pad, w + 2 * pad, x.device, x.dtype)
    check(lib.sscg_reflect_pad(x.data_ptr(), y.data_ptr(), _dt(x), n, h, w, c, pad, _stream()), "sscg_reflect_pad")
    return y


def reflect_pad_bwd(dy, pad):
    n, c, oh, ow = dy.shape
    dx = empty_nhwc(n, c, oh - 2 * pad, ow - 2 * pad, dy.device, dy.dtype)
    check(lib.sscg_reflect_pad_bwd(dy.data_ptr(), dx.data_ptr(), _dt(dy), n, oh - 2 * pad, ow - 2 * pad, c, pad, _stream()),
          "sscg_reflect_pad_bwd")
    return dx


def softmax_fwd(x):
    _need_hip(x, f32_only=True)
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=CL)
    check(lib.sscg_softmax_fwd(x.data_ptr(), y.data_ptr(), n * h * w, c, _stream()), "sscg_softmax_fwd")
    return y


def softmax_bwd(dy, y):
    n, c, h, w = y.shape
    dx = torch.empty_like(y, memory_format=CL)
    check(lib.sscg_softmax_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), n * h * w, c, _stream()), "sscg_softmax_bwd")
    return dx


def argmax_onehot(x, want_index=False):
    """`x.max(1)[1]` + make_one_hot in one pass (model.py:435-437).  Returns (onehot NHWC, index [N,H,W] or None)."""
    _need_hip(x, f32_only=True)
    x = to_nhwc(x)
    n, c, h, w = x.shape
    oh = torch.empty_like(x, memory_format=CL)
    idx = torch.empty((n, h, w), dtype=torch.int64, device=x.device) if want_index else None
    check(lib.sscg_argmax_onehot(x.data_ptr(), oh.data_ptr(), _ptr(idx), n * h * w, c, _stream()), "sscg_argmax_onehot")
    return oh, idx


def argmax_index(x):
    _need_hip(x, f32_only=True)
    x = to_nhwc(x)
    n, c, h, w = x.shape
    idx = torch.empty((n, h, w), dtype=torch.int64, device=x.device)
    check(lib.sscg_argmax_onehot(x.data_ptr(), None, idx.data_ptr(), n * h * w, c, _stream()), "sscg_argmax_onehot")
    return idx


def confusion_hist(label_true, label_pred, num_classes, hist=None):
    """hist[C*t + p] += 1 over the pixels with 0 <= t < C (utils.py:363-369); `hist` int64 [C, C] on the device."""
    if not (label_true.is_cuda and label_pred.is_cuda):
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
    lt = label_true.to(torch.int64).contiguous()
    lp = label_pred.to(torch.int64).contiguous()
    if lt.numel() != lp.numel():
        raise _lib.SscgError("confusion_hist: label/prediction sizes differ")
    if hist is None:
        hist = torch.empty((num_classes, num_classes), dtype=torch.int64, device=lt.device)
        check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
    check(lib.sscg_confusion_hist(lt.data_ptr(), lp.data_ptr(), lt.numel(), num_classes, hist.data_ptr(), _stream()),
          "sscg_confusion_hist")
    return hist


def label_hist(labels, num_classes, counts=None):
    """counts[c] += #{labels == c}; ids outside [0, C) are ignored.  `counts` int64 [C] on the device (exact: integer atomics) - the
    class frequencies the weight rules of the class-weighted cross entropy start from (utils.ce_weights_from_counts)."""
    if not labels.is_cuda:
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % labels.device)
    lab = labels.to(torch.int64).contiguous()
    if counts is None:
        counts = torch.empty((num_classes,), dtype=torch.int64, device=lab.device)
        check(lib.sscg_fill(counts.data_ptr(), 2 * counts.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
    check(lib.sscg_label_hist(lab.data_ptr(), lab.numel(), num_classes, counts.data_ptr(), _stream()), "sscg_label_hist")
    return counts


# The inference heads (sscg_predict_head / sscg_image_head): what evaluate(), validation.py and testing.py keep of a generator's
# output, in one launch.  SSCG_FUSE_PREDICT=0 keeps those call sites on the chain of separate passes (an A/B aid: the bits are the same).
FUSE_PREDICT = [os.environ.get("SSCG_FUSE_PREDICT", "1") != "0"]


def _no_grad_input(x, what):
    if x.requires_grad and torch.is_grad_enabled():
        raise _lib.SscgError("%s is an inference call, not an autograd node: call it under torch.no_grad() or on a detached tensor" % what)


def predict_labels(logits, size, *, want_index=False, want_u8=True, label_true=None, hist=None, num_classes=None):
    """interp(size, bilinear, align_corners=True) -> Softmax2d -> .max(1)[1] of fp32 logits [N,C,H,W] in one launch, bit for bit what
    `argmax_index(softmax2d(upsample_bilinear(logits, size)))` gives (model.py:555-574, validation.py:97-120, testing.py:43).
    Returns (label_u8 uint8 [N,OH,OW] or None, index int64 [N,OH,OW] or None, hist or None).  `label_true` (int64, N*OH*OW elements)
    adds the batch to the confusion matrix `hist` (int64 [C,C] on the device, runningScore._fast_hist's rules; None = a new zeroed one)."""
    _need_hip(logits, f32_only=True)
    if logits.dim() != 4:
        raise _lib.SscgError("predict_labels: 4-D logits expected")
    _no_grad_input(logits, "predict_labels")
    x = to_nhwc(logits.detach())
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    if num_classes is not None and int(num_classes) != c:
        raise _lib.SscgError("predict_labels: %d classes asked for, the logits have %d channels" % (num_classes, c))
    if hist is not None and label_true is None:
        raise _lib.SscgError("predict_labels: a confusion matrix needs label_true")
    lt = None
    if label_true is not None:
        if not label_true.is_cuda:
            raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
        lt = label_true.to(torch.int64).contiguous()
        if lt.numel() != n * oh * ow:
            raise _lib.SscgError("predict_labels: label_true must have N*OH*OW elements")
        if hist is None:
            hist = torch.empty((c, c), dtype=torch.int64, device=x.device)
            check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
        elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == c * c):
            raise _lib.SscgError("predict_labels: hist must be a contiguous int64 [C, C] tensor on the device")
    u8 = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device) if want_u8 else None
    idx = torch.empty((n, oh, ow), dtype=torch.int64, device=x.device) if want_index else None
    check(lib.sscg_predict_head(x.data_ptr(), n, h, w, c, oh, ow, _ptr(idx), _ptr(u8), _ptr(lt), _ptr(hist), _stream()),
          "sscg_predict_head")
    return u8, idx, hist


def predict_image(x, size, *, want_float=True, want_u8=True):
    """interp(size) -> Tanh of the image generator's fp32 output [N,C,H,W] (C <= 4) in one launch (validation.py:108-114).  Returns
    (y, rgb_u8): y = fp32 [N,C,OH,OW] channels-last, bit for bit `act_fwd(to_nhwc(upsample_bilinear(x, size)), ACT_TANH)`; rgb_u8 =
    uint8 [N,OH,OW,C], the pixels `save_image(y * 0.5 + 0.5)` writes (x * 255 + 0.5, clamp, truncate; every step rounded to fp32)."""
    _need_hip(x, f32_only=True)
    if x.dim() != 4:
        raise _lib.SscgError("predict_image: 4-D tensor expected")
    _no_grad_input(x, "predict_image")
    x = to_nhwc(x.detach())
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    y = empty_nhwc(n, c, oh, ow, x.device) if want_float else None
    u8 = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device) if want_u8 else None
    check(lib.sscg_image_head(x.data_ptr(), n, h, w, c, oh, ow, _ptr(y), _ptr(u8), _stream()), "sscg_image_head")
    return y, u8


# Multi-scale / mirrored inference (sscg_predict_head_ms / sscg_resize_flip): the logit maps of several views of one batch fused into
# one label map in one launch.  SSCG_FUSE_TTA=0 keeps predict_labels_ms on the chain of separate passes (an A/B aid: the bits are the
# same).
FUSE_TTA = [os.environ.get("SSCG_FUSE_TTA", "1") != "0"]
MAX_VIEWS = 8


def resize_flip(x, size, flip):
    """The network input of one view: `upsample_bilinear(x, size)` (bilinear, align_corners=True; a smaller size samples), then
    `torch.flip` of the W axis when `flip` - one launch, the same bits.  fp32 [N,C,H,W] in, channels-last out; the batch itself when
    there is nothing to do."""
    _need_hip(x, f32_only=True)
    if x.dim() != 4:
        raise _lib.SscgError("resize_flip: 4-D tensor expected")
    _no_grad_input(x, "resize_flip")
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    if not flip and (oh, ow) == (h, w):
        return x
    x = to_nhwc(x.detach())
    y = empty_nhwc(n, c, oh, ow, x.device)
    check(lib.sscg_resize_flip(x.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow, 1 if flip else 0, _stream()), "sscg_resize_flip")
    return y


def mirror_samples(x, flags):
    """The batch x [N,C,H,W] (fp32, no gradient) with sample n mirrored on W where flags[n] (a host sequence of N booleans) is set, as a
    new channels-last tensor: per run of equal flags one sscg_resize_flip launch at the samples' own size (mirrored runs) or one copy
    (plain runs), straight into the run's slice of the result - every sample is read and written once.  The batch itself when no flag
    is set."""
    _need_hip(x, f32_only=True)
    if x.dim() != 4:
        raise _lib.SscgError("mirror_samples: 4-D tensor expected")
    _no_grad_input(x, "mirror_samples")
    flags = [bool(f) for f in flags]
    n, c, h, w = x.shape
    if len(flags) != n:
        raise ValueError("mirror_samples: %d flags for a batch of %d" % (len(flags), n))
    if not any(flags):
        return x
    x = to_nhwc(x.detach())
    y = empty_nhwc(n, c, h, w, x.device)
    n0 = 0
    while n0 < n:
        n1 = n0 + 1
        while n1 < n and flags[n1] == flags[n0]:
            n1 += 1
        if flags[n0]:
            check(lib.sscg_resize_flip(x[n0:n1].data_ptr(), y[n0:n1].data_ptr(), n1 - n0, h, w, c, h, w, 1, _stream()), "sscg_resize_flip")
        else:
            y[n0:n1].copy_(x[n0:n1])
        n0 = n1
    return y


def mix_table_rows(table, n):
    """A host mix table (numpy or CPU tensor, data_utils.augmentations.Compose.mixes' int32 [N, 8] rows) as a contiguous int32 CPU
    tensor, checked: the shape, and the class-mask words, which the box entries do not read and therefore refuse when set."""
    t = torch.as_tensor(table)
    if t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (n, 8):
        raise _lib.SscgError("a host int32 [%d, 8] mix table expected, got %s %s on %s" % (n, t.dtype, tuple(t.shape), t.device))
    if bool((t[:, 5:7] != 0).any()):
        raise ValueError("the mix table names class masks (words 5 and 6): the box entries mix boxes only - ClassMix is "
                         "functional.augment_batch(mix=)'s")
    return t.contiguous()


def mix_rows_live(rows):
    """Which rows of a checked host table can paste anything (bool [N]): a partner in [0, N) other than the sample, a non-empty box"""
    n = rows.shape[0]
    idx = torch.arange(n, dtype=torch.int32)
    p = rows[:, 0]
    return (p >= 0) & (p < n) & (p != idx) & (rows[:, 1] < rows[:, 3]) & (rows[:, 2] < rows[:, 4])


def upload_mix_table(rows, device):
    """The checked host table on `device`, through pinned memory: nothing waits for the copy"""
    return (rows.pin_memory() if device.type == "cuda" else rows).to(device, non_blocking=True)


def mix_boxes(x, table, device_table=None):
    """CutMix of a finished batch (sscg_mix_boxes, one launch): x fp32 [N,C,H,W] (no gradient), table a HOST int32 [N, 8] (numpy or CPU
    tensor; data_utils.augmentations.Compose.mixes' rows, class-mask words 0) -> a new channels-last tensor with sample n's box taken
    from sample table[n][0] - data_utils.augmentations.mix_batch(x, None, table, False) bit for bit.  The batch itself when no row
    mixes.  `device_table`: the table already on x's device (upload_mix_table), else it is uploaded here without a sync."""
    if x.dim() != 4:
        raise _lib.SscgError("mix_boxes: 4-D tensor expected")
    n, c, h, w = x.shape
    rows = mix_table_rows(table, n)         # (the table's own errors first: they need no device)
    _need_hip(x, f32_only=True)
    _no_grad_input(x, "mix_boxes")
    if not bool(mix_rows_live(rows).any()):
        return x
    x = to_nhwc(x.detach())
    y = empty_nhwc(n, c, h, w, x.device)
    dt = device_table if device_table is not None else upload_mix_table(rows, x.device)
    check(lib.sscg_mix_boxes(x.data_ptr(), y.data_ptr(), dt.data_ptr(), n, h, w, c, _stream()), "sscg_mix_boxes")
    return y


def predict_labels_ms(logits_list, flips, size, *, want_prob=False, want_index=False, want_u8=True, label_true=None, hist=None,
                      num_classes=None):
    """Label maps from the logits of up to 8 views of one batch: per view, in order, interp(size, bilinear, align_corners=True) ->
    mirror of the W axis where `flips[s]` (the view was computed from the mirrored image) -> Softmax2d, the views' probabilities
    summed in fp32 (no division by their number), then .max(1)[1] - one launch, bit for bit what the separate passes give.
    Returns (label_u8 uint8 [N,OH,OW] or None, index int64 [N,OH,OW] or None, hist or None, prob_sum fp32 [N,C,OH,OW] channels-last
    or None); `label_true` / `hist` as in predict_labels."""
    S = len(logits_list)
    if not 1 <= S <= MAX_VIEWS or len(flips) != S:
        raise _lib.SscgError("predict_labels_ms: 1..%d views with one flip flag each expected" % MAX_VIEWS)
    xs = []
    for lg in logits_list:
        _need_hip(lg, f32_only=True)
        if lg.dim() != 4 or lg.shape[:2] != logits_list[0].shape[:2]:
            raise _lib.SscgError("predict_labels_ms: 4-D logits of one batch size and class count expected")
        _no_grad_input(lg, "predict_labels_ms")
        xs.append(to_nhwc(lg.detach()))
    n, c = xs[0].shape[:2]
    oh, ow = int(size[0]), int(size[1])
    if num_classes is not None and int(num_classes) != c:
        raise _lib.SscgError("predict_labels_ms: %d classes asked for, the logits have %d channels" % (num_classes, c))
    if hist is not None and label_true is None:
        raise _lib.SscgError("predict_labels_ms: a confusion matrix needs label_true")
    if not (want_prob or want_index or want_u8 or label_true is not None):
        raise _lib.SscgError("predict_labels_ms: no output asked for")
    lt = None
    if label_true is not None:
        if not label_true.is_cuda:
            raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
        lt = label_true.to(torch.int64).contiguous()
        if lt.numel() != n * oh * ow:
            raise _lib.SscgError("predict_labels_ms: label_true must have N*OH*OW elements")
        if hist is None:
            hist = torch.empty((c, c), dtype=torch.int64, device=xs[0].device)
            check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
        elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == c * c):
            raise _lib.SscgError("predict_labels_ms: hist must be a contiguous int64 [C, C] tensor on the device")
    if not FUSE_TTA[0]:
        acc = None
        for x, flip in zip(xs, flips):
            p = softmax_fwd(x if tuple(x.shape[2:]) == (oh, ow) else upsample_fwd(x, oh, ow))      # a fresh tensor per view
            if flip:
                p = torch.flip(p, dims=(3,))
            acc = p if acc is None else acc.add_(p)
        idx = argmax_index(acc) if (want_index or want_u8 or lt is not None) else None
        if lt is not None:
            confusion_hist(lt, idx, c, hist)
        return (idx.to(torch.uint8) if want_u8 else None, idx if want_index else None, hist,
                acc.contiguous(memory_format=CL) if want_prob else None)
    u8 = torch.empty((n, oh, ow), dtype=torch.uint8, device=xs[0].device) if want_u8 else None
    idx = torch.empty((n, oh, ow), dtype=torch.int64, device=xs[0].device) if want_index else None
    prob = empty_nhwc(n, c, oh, ow, xs[0].device) if want_prob else None
    mask = 0
    for s, flip in enumerate(flips):
        mask |= (1 if flip else 0) << s
    ptrs = (C.c_void_p * S)(*[x.data_ptr() for x in xs])
    hs = (C.c_int * S)(*[int(x.shape[2]) for x in xs])
    ws = (C.c_int * S)(*[int(x.shape[3]) for x in xs])
    check(lib.sscg_predict_head_ms(ptrs, hs, ws, S, mask, n, c, oh, ow, _ptr(prob), _ptr(idx), _ptr(u8), _ptr(lt), _ptr(hist), _stream()),
          "sscg_predict_head_ms")
    return u8, idx, hist, prob


# Sliding-window inference (sscg_window_gather / sscg_predict_head_sw, include/sscg.h holds the definition): the network on overlapping
# windows of its training size over a larger image, the windows' probabilities blended into one label map in one launch.  Opt-in
# (`--sliding`).  SSCG_FUSE_SLIDING=0 keeps window_gather / predict_labels_sw on the chains of separate passes (an A/B aid: the bits are
# the same).
FUSE_SLIDING = [os.environ.get("SSCG_FUSE_SLIDING", "1") != "0"]
SLIDING_MAX_WINDOWS = 16        # per axis


class SlidingOptions(object):
    """`window` = (wh, ww), the size the network was trained at; `size` = (H, W) >= window, the evaluation size the images are kept at;
    `overlap` in [0, 0.75] of the window shared by neighbours; `blend` = "gauss" (weights exp(-d^2 / (2 (sigma w)^2)) around the
    window's centre, `sigma` in (0, 1] of the window; 0.125 is MONAI's / nnU-Net's value, untuned here) or "const"; `flip`: every window
    also runs mirrored along W."""
    __slots__ = ("window", "size", "overlap", "blend", "sigma", "flip")

    def __init__(self, window, size, overlap=0.5, blend="gauss", sigma=0.125, flip=False):
        try:
            window, size = (int(window[0]), int(window[1])), (int(size[0]), int(size[1]))
        except (TypeError, ValueError, IndexError):
            raise ValueError("sliding: window and size are (height, width) pairs, got %r and %r" % (window, size))
        if window[0] < 1 or window[1] < 1:
            raise ValueError("sliding window %r is not positive" % (window,))
        if size[0] < window[0] or size[1] < window[1]:
            raise ValueError("sliding size %dx%d is below the %dx%d window (the crop)" % (size + window))
        overlap, sigma = float(overlap), float(sigma)
        if not 0.0 <= overlap <= 0.75:
            raise ValueError("sliding overlap %r is outside [0, 0.75]" % (overlap,))
        if blend not in ("gauss", "const"):
            raise ValueError("sliding blend %r is neither gauss nor const" % (blend,))
        if not 0.0 < sigma <= 1.0:
            raise ValueError("sliding sigma %r is outside (0, 1]" % (sigma,))
        self.window, self.size, self.overlap, self.blend, self.sigma, self.flip = window, size, overlap, blend, sigma, bool(flip)
        for L, w in zip(size, window):
            if len(sliding_positions(L, w, overlap)) > SLIDING_MAX_WINDOWS:
                raise ValueError("sliding: %d windows of %d along an axis of %d at overlap %r, at most %d" % (
                    len(sliding_positions(L, w, overlap)), w, L, overlap, SLIDING_MAX_WINDOWS))

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, SlidingOptions) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "SlidingOptions(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def sliding_stride(w, overlap):
    return max(1, int(w * (1.0 - overlap) + 0.5))


def sliding_positions(L, w, overlap):
    """The window positions along an axis of length L: stride s = max(1, int(w (1 - overlap) + 0.5)), k = 1 if L == w else
    ceil((L - w) / s) + 1 windows at min(i s, L - w) - the last one pushed back flush with the edge."""
    L, w = int(L), int(w)
    if w > L:
        raise ValueError("sliding: a window of %d does not fit an axis of %d" % (w, L))
    s = sliding_stride(w, overlap)
    k = 1 if L == w else -(-(L - w) // s) + 1
    return [min(i * s, L - w) for i in range(k)]


def _sliding_tables(L, w, pos, blend, sigma):
    """(weights fp32 [w], reciprocal coverage fp32 [L]) of one axis: the weights computed in float64 and rounded once; the coverage
    summed in fp32 in ascending window order."""
    import numpy as np
    if blend == "gauss":
        d = np.arange(w, dtype=np.float64) - (w - 1) / 2.0
        wt = np.exp(-(d * d) / (2.0 * (sigma * w) ** 2)).astype(np.float32)
    else:
        wt = np.ones(w, dtype=np.float32)
    cov = np.zeros(L, dtype=np.float32)
    for p in pos:
        cov[p:p + w] += wt
    return wt, (np.float32(1) / cov).astype(np.float32)


class SlidingPlan(object):
    """The geometry of one (H, W, options): per axis the stride, the window count and positions, the weight table and the normaliser;
    `views` = windows per sample x (2 with flip).  With a device: the four tables as fp32 tensors there (uploaded once)."""
    __slots__ = ("options", "OH", "OW", "wh", "ww", "sy", "sx", "ky", "kx", "pos_y", "pos_x", "flip", "views", "wy", "wx", "ry", "rx",
                 "device", "wy_dev", "wx_dev", "ry_dev", "rx_dev")

    def single(self):
        """One unmirrored window: the image is the window."""
        return self.views == 1


_SLIDING_PLANS = {}


def sliding_plan(H, W, options, device=None):
    """The SlidingPlan of images [H, W] under `options`, cached per (H, W, options, device).  `device` None: host tables only."""
    import numpy as np
    if not isinstance(options, SlidingOptions):
        raise TypeError("sliding_plan: a functional.SlidingOptions expected, not %r" % (options,))
    H, W = int(H), int(W)
    key = (H, W, options, None if device is None else str(device))
    plan = _SLIDING_PLANS.get(key)
    if plan is not None:
        return plan
    wh, ww = options.window
    if H < wh or W < ww:
        raise ValueError("sliding: images of %dx%d are below the %dx%d window" % (H, W, wh, ww))
    plan = SlidingPlan()
    plan.options, plan.OH, plan.OW, plan.wh, plan.ww, plan.flip = options, H, W, wh, ww, options.flip
    plan.sy, plan.sx = sliding_stride(wh, options.overlap), sliding_stride(ww, options.overlap)
    plan.pos_y, plan.pos_x = sliding_positions(H, wh, options.overlap), sliding_positions(W, ww, options.overlap)
    plan.ky, plan.kx = len(plan.pos_y), len(plan.pos_x)
    if max(plan.ky, plan.kx) > SLIDING_MAX_WINDOWS:
        raise ValueError("sliding: %d x %d windows over %dx%d, at most %d per axis" % (plan.ky, plan.kx, H, W, SLIDING_MAX_WINDOWS))
    plan.views = plan.ky * plan.kx * (2 if plan.flip else 1)
    plan.wy, plan.ry = _sliding_tables(H, wh, plan.pos_y, options.blend, options.sigma)
    plan.wx, plan.rx = _sliding_tables(W, ww, plan.pos_x, options.blend, options.sigma)
    if plan.flip:
        plan.ry = plan.ry * np.float32(0.5)         # the two views of a window carry the same weight
    plan.device = device
    plan.wy_dev = plan.wx_dev = plan.ry_dev = plan.rx_dev = None
    if device is not None:
        plan.wy_dev, plan.wx_dev, plan.ry_dev, plan.rx_dev = (torch.from_numpy(np.ascontiguousarray(t)).to(device)
                                                              for t in (plan.wy, plan.wx, plan.ry, plan.rx))
    _SLIDING_PLANS[key] = plan
    return plan


def _plan_on(plan, t, what):
    if not isinstance(plan, SlidingPlan):
        raise TypeError("%s: a plan of functional.sliding_plan expected, not %r" % (what, plan))
    if plan.wy_dev is None or plan.wy_dev.device != t.device:
        raise _lib.SscgError("%s: the plan's tables are not on %s (sliding_plan(..., device=))" % (what, t.device))


def window_gather(images, plan):
    """The network input of every window of `plan`: fp32 [N,C,H,W] -> channels-last [N * views, C, wh, ww], window
    ((n ky + iy) kx + ix) F + f, the f = 1 twin with its columns mirrored - a pure copy in one launch; the batch itself when there is
    one unmirrored window."""
    _need_hip(images, f32_only=True)
    if images.dim() != 4:
        raise _lib.SscgError("window_gather: 4-D tensor expected")
    _no_grad_input(images, "window_gather")
    if not isinstance(plan, SlidingPlan):
        raise TypeError("window_gather: a plan of functional.sliding_plan expected, not %r" % (plan,))
    n, c, h, w = images.shape
    if (h, w) != (plan.OH, plan.OW):
        raise _lib.SscgError("window_gather: images of %dx%d, the plan is for %dx%d" % (h, w, plan.OH, plan.OW))
    if plan.single():
        return images
    if not FUSE_SLIDING[0]:
        x = images.detach()
        wins = []
        for i in range(n):
            for py in plan.pos_y:
                for px in plan.pos_x:
                    t = x[i, :, py:py + plan.wh, px:px + plan.ww]
                    wins.append(t)
                    if plan.flip:
                        wins.append(torch.flip(t, dims=(2,)))
        return torch.stack(wins).contiguous(memory_format=CL)
    x = to_nhwc(images.detach())
    y = empty_nhwc(n * plan.views, c, plan.wh, plan.ww, x.device)
    check(lib.sscg_window_gather(x.data_ptr(), y.data_ptr(), n, h, w, c, plan.wh, plan.ww, plan.sy, plan.sx, plan.ky, plan.kx,
                                 1 if plan.flip else 0, _stream()), "sscg_window_gather")
    return y


def predict_labels_sw(logits, plan, *, want_prob=False, want_index=False, want_u8=True, label_true=None, hist=None, num_classes=None):
    """Label maps at the plan's evaluation size from the logits of its windows, fp32 [N * views, C, h, w] in window_gather's order: per
    output pixel, over the windows that cover it in ascending order (the unmirrored view before the mirrored one), interp(window,
    bilinear, align_corners=True) -> mirror -> Softmax2d, times the window's blend weight, summed in fp32; then .max(1)[1] - one
    launch, bit for bit what the separate passes give.  Returns (label_u8 uint8 [N,OH,OW] or None, index int64 [N,OH,OW] or None,
    hist or None, prob fp32 [N,C,OH,OW] channels-last or None = the blended, NORMALISED probabilities); `label_true` / `hist` as in
    predict_labels."""
    _need_hip(logits, f32_only=True)
    if logits.dim() != 4:
        raise _lib.SscgError("predict_labels_sw: 4-D logits expected")
    _no_grad_input(logits, "predict_labels_sw")
    _plan_on(plan, logits, "predict_labels_sw")
    x = to_nhwc(logits.detach())
    nv, c, h, w = x.shape
    if nv % plan.views:
        raise _lib.SscgError("predict_labels_sw: %d logit maps are no multiple of the plan's %d windows per sample" % (nv, plan.views))
    n, oh, ow = nv // plan.views, plan.OH, plan.OW
    if num_classes is not None and int(num_classes) != c:
        raise _lib.SscgError("predict_labels_sw: %d classes asked for, the logits have %d channels" % (num_classes, c))
    if hist is not None and label_true is None:
        raise _lib.SscgError("predict_labels_sw: a confusion matrix needs label_true")
    if not (want_prob or want_index or want_u8 or label_true is not None):
        raise _lib.SscgError("predict_labels_sw: no output asked for")
    lt = None
    if label_true is not None:
        if not label_true.is_cuda:
            raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
        lt = label_true.to(torch.int64).contiguous()
        if lt.numel() != n * oh * ow:
            raise _lib.SscgError("predict_labels_sw: label_true must have N*OH*OW elements")
        if hist is None:
            hist = torch.empty((c, c), dtype=torch.int64, device=x.device)
            check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
        elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == c * c):
            raise _lib.SscgError("predict_labels_sw: hist must be a contiguous int64 [C, C] tensor on the device")
    if not FUSE_SLIDING[0]:
        acc = torch.zeros((n, c, oh, ow), dtype=torch.float32, device=x.device).contiguous(memory_format=CL)
        blend = plan.wy_dev[:, None] * plan.wx_dev[None, :]
        F_ = 2 if plan.flip else 1
        for iy, py in enumerate(plan.pos_y):
            for ix, px in enumerate(plan.pos_x):
                for f in range(F_):
                    xk = to_nhwc(x[(iy * plan.kx + ix) * F_ + f::plan.views])           # the window's map of every sample
                    p = softmax_fwd(xk if (h, w) == (plan.wh, plan.ww) else upsample_fwd(xk, plan.wh, plan.ww))
                    if f:
                        p = torch.flip(p, dims=(3,))
                    acc[:, :, py:py + plan.wh, px:px + plan.ww].add_(torch.mul(p, blend))
        idx = argmax_index(acc) if (want_index or want_u8 or lt is not None) else None
        if lt is not None:
            confusion_hist(lt, idx, c, hist)
        prob = (acc * (plan.ry_dev[:, None] * plan.rx_dev[None, :])).contiguous(memory_format=CL) if want_prob else None
        return idx.to(torch.uint8) if want_u8 else None, idx if want_index else None, hist, prob
    u8 = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device) if want_u8 else None
    idx = torch.empty((n, oh, ow), dtype=torch.int64, device=x.device) if want_index else None
    prob = empty_nhwc(n, c, oh, ow, x.device) if want_prob else None
    check(lib.sscg_predict_head_sw(x.data_ptr(), n, h, w, c, plan.wh, plan.ww, plan.sy, plan.sx, plan.ky, plan.kx, 1 if plan.flip else 0,
                                   oh, ow, plan.wy_dev.data_ptr(), plan.wx_dev.data_ptr(), plan.ry_dev.data_ptr(), plan.rx_dev.data_ptr(),
                                   _ptr(prob), _ptr(idx), _ptr(u8), _ptr(lt), _ptr(hist), _stream()), "sscg_predict_head_sw")
    return u8, idx, hist, prob


# Windowed dense-CRF refinement of a predicted class map (sscg_crf_head, include/sscg.h holds the definition): opt-in (`--crf`), an
# inference call.  The defaults below are UNTUNED - no dataset was on hand to tune them; theta_beta is in the units of the guide image
# the drivers pass, the normalised batch.
class CrfOptions(object):
    """iterations >= 0 mean-field steps over a dilated (2 radius + 1)^2 window (radius 1..5, dilation >= 1, radius * dilation <= 16);
    w_bilateral / w_spatial finite and >= 0; theta_alpha / theta_beta / theta_gamma > 0."""
    __slots__ = ("iterations", "radius", "dilation", "w_bilateral", "w_spatial", "theta_alpha", "theta_beta", "theta_gamma")

    def __init__(self, iterations=5, radius=3, dilation=2, w_bilateral=4.0, w_spatial=3.0, theta_alpha=8.0, theta_beta=0.5,
                 theta_gamma=3.0):
        for name, val in (("iterations", iterations), ("radius", radius), ("dilation", dilation)):
            if isinstance(val, bool) or not isinstance(val, (int, float)) or not abs(val) < 2 ** 31 or val != int(val):
                raise ValueError("crf %s %r is not an integer" % (name, val))
        it, r, d = int(iterations), int(radius), int(dilation)
        if it < 0:
            raise ValueError("crf iterations %r is not an integer >= 0" % (iterations,))
        if not 1 <= r <= 5:
            raise ValueError("crf radius %r is outside 1..5" % (radius,))
        if d < 1 or r * d > 16:
            raise ValueError("crf dilation %r: at least 1, and radius * dilation at most 16" % (dilation,))
        ws = {}
        for name, val in (("w_bilateral", w_bilateral), ("w_spatial", w_spatial)):
            ws[name] = float(val)
            if not (ws[name] >= 0.0 and ws[name] < float("inf")):
                raise ValueError("crf %s %r is not a finite number >= 0" % (name, val))
        for name, val in (("theta_alpha", theta_alpha), ("theta_beta", theta_beta), ("theta_gamma", theta_gamma)):
            ws[name] = float(val)
            if not ws[name] > 0.0:
                raise ValueError("crf %s %r is not > 0" % (name, val))
        self.iterations, self.radius, self.dilation = it, r, d
        for name, val in ws.items():
            setattr(self, name, val)

    def params(self):
        return _lib.CrfParams(self.radius, self.dilation, self.iterations, self.w_bilateral, self.w_spatial, self.theta_alpha,
                              self.theta_beta, self.theta_gamma)

    def __eq__(self, other):
        return isinstance(other, CrfOptions) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __repr__(self):
        return "CrfOptions(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


_CRF_WS_BYTES = {}


def crf_labels(x, image, size, crf, *, probs=False, want_q=False, want_index=False, want_u8=True, label_true=None, hist=None,
               num_classes=None):
    """Label maps after `crf.iterations` mean-field steps of the windowed dense CRF (sscg_crf_head).  `x`: fp32 [N,C,H,W] logits,
    resized to `size` like predict_labels' - or, with probs=True, non-negative scores already at `size` (prob_sum of predict_labels_ms).
    `image`: the guide, fp32 [N,IC,OH,OW] at `size`, IC <= 4.  Returns (label_u8 uint8 [N,OH,OW] or None, index int64 [N,OH,OW] or None,
    hist or None, q fp32 [N,C,OH,OW] channels-last or None = Q after the last step); `label_true` / `hist` as in predict_labels.
    iterations == 0 is predict_labels (logits) / the first maximum of the scores, bit for bit; it has no q."""
    if not isinstance(crf, CrfOptions):
        raise TypeError("crf must be a functional.CrfOptions, not %r" % (crf,))
    _need_hip(x, f32_only=True)
    _need_hip(image, f32_only=True)
    if x.dim() != 4 or image.dim() != 4:
        raise _lib.SscgError("crf_labels: 4-D scores and a 4-D guide image expected")
    _no_grad_input(x, "crf_labels")
    _no_grad_input(image, "crf_labels")
    xs = to_nhwc(x.detach())
    n, c, h, w = xs.shape
    oh, ow = int(size[0]), int(size[1])
    if tuple(image.shape) != (n, image.shape[1], oh, ow) or not 1 <= image.shape[1] <= 4:
        raise _lib.SscgError("crf_labels: the guide image must be [N, 1..4, OH, OW] at the output size, got %s" % (tuple(image.shape),))
    if probs and (h, w) != (oh, ow):
        raise _lib.SscgError("crf_labels: scores (probs=True) must already have the output size")
    if num_classes is not None and int(num_classes) != c:
        raise _lib.SscgError("crf_labels: %d classes asked for, the scores have %d channels" % (num_classes, c))
    if hist is not None and label_true is None:
        raise _lib.SscgError("crf_labels: a confusion matrix needs label_true")
    if not (want_q or want_index or want_u8 or label_true is not None):
        raise _lib.SscgError("crf_labels: no output asked for")
    if want_q and crf.iterations == 0:
        raise _lib.SscgError("crf_labels: Q is the result of a mean-field step, iterations == 0 has none")
    guide = to_nhwc(image.detach())
    lt = None
    if label_true is not None:
        if not label_true.is_cuda:
            raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
        lt = label_true.to(torch.int64).contiguous()
        if lt.numel() != n * oh * ow:
            raise _lib.SscgError("crf_labels: label_true must have N*OH*OW elements")
        if hist is None:
            hist = torch.empty((c, c), dtype=torch.int64, device=xs.device)
            check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
        elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == c * c):
            raise _lib.SscgError("crf_labels: hist must be a contiguous int64 [C, C] tensor on the device")
    u8 = torch.empty((n, oh, ow), dtype=torch.uint8, device=xs.device) if want_u8 else None
    idx = torch.empty((n, oh, ow), dtype=torch.int64, device=xs.device) if want_index else None
    q = empty_nhwc(n, c, oh, ow, xs.device) if want_q else None
    key = (n, c, oh, ow, crf.iterations)
    if key not in _CRF_WS_BYTES:
        _CRF_WS_BYTES[key] = lib.sscg_crf_workspace(*key)
    ws = _WS.get(_CRF_WS_BYTES[key], xs.device)
    check(lib.sscg_crf_head(xs.data_ptr(), _lib.CRF_PROBS if probs else _lib.CRF_LOGITS, n, h, w, c, oh, ow, guide.data_ptr(),
                            int(guide.shape[1]), C.byref(crf.params()), _ptr(q), _ptr(idx), _ptr(u8), _ptr(lt), _ptr(hist), ws.data_ptr(),
                            ws.numel(), _stream()), "sscg_crf_head")
    return u8, idx, hist, q


# Contour scores of the evaluation (sscg_boundary_counts, include/sscg.h holds the definitions): opt-in (`--boundary`).
BOUNDARY_MAX_D = 32


class BoundaryOptions(object):
    """The contour width of the Boundary IoU / trimap mIoU: `d` pixels (1..32, chessboard metric) given directly, or `ratio` of the
    image diagonal (in (0, 1]; the published default 0.02) - one of the two, never both."""
    __slots__ = ("d", "ratio")

    def __init__(self, d=None, ratio=None):
        if d is not None and ratio is not None:
            raise ValueError("boundary: d and ratio are two ways to give one width, got both")
        if d is not None:
            if isinstance(d, bool) or not isinstance(d, (int, float)) or d != d or d != int(d) or not 1 <= int(d) <= BOUNDARY_MAX_D:
                raise ValueError("boundary d %r is not an integer in 1..%d" % (d, BOUNDARY_MAX_D))
            d = int(d)
        else:
            ratio = 0.02 if ratio is None else ratio
            if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) <= 1.0:
                raise ValueError("boundary ratio %r is not a number in (0, 1]" % (ratio,))
            ratio = float(ratio)
        self.d, self.ratio = d, ratio

    def width(self, h, w):
        """The width in pixels on an h x w map: d itself, or max(1, int(ratio * diagonal + 0.5)); above 32 is refused."""
        if self.d is not None:
            return self.d
        d = max(1, int(self.ratio * (float(h) * h + float(w) * w) ** 0.5 + 0.5))
        if d > BOUNDARY_MAX_D:
            raise ValueError("boundary width d = %d (ratio %g of the diagonal of a %d x %d map) is above %d" % (
                d, self.ratio, h, w, BOUNDARY_MAX_D))
        return d

    def __eq__(self, other):
        return isinstance(other, BoundaryOptions) and (self.d, self.ratio) == (other.d, other.ratio)

    def __repr__(self):
        return "BoundaryOptions(d=%r, ratio=%r)" % (self.d, self.ratio)


def boundary_counts(label_true, label_pred, num_classes, d, counts=None):
    """The counts behind the Boundary IoU and the trimap mIoU of a batch (sscg_boundary_counts): label_true [N,H,W] (any integer
    type, values outside [0, C) are void), label_pred [N,H,W] class ids as bytes, width d in 1..32.  Returns `counts`, int64
    [3 C + C C] on the device = bt | bp | bi | tri, accumulated into (None = a new zeroed one)."""
    if not (label_true.is_cuda and label_pred.is_cuda):
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
    if isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= BOUNDARY_MAX_D:
        raise ValueError("boundary_counts: d = %r is not an integer in 1..%d" % (d, BOUNDARY_MAX_D))
    c = int(num_classes)
    if label_true.dim() != 3 or tuple(label_true.shape) != tuple(label_pred.shape):
        raise _lib.SscgError("boundary_counts: two [N, H, W] label maps of one shape expected, got %s and %s" % (
            tuple(label_true.shape), tuple(label_pred.shape)))
    lt = label_true.to(torch.int64).contiguous()
    lp = label_pred.to(torch.uint8).contiguous()
    nb = 3 * c + c * c
    if counts is None:
        counts = torch.empty((nb,), dtype=torch.int64, device=lt.device)
        check(lib.sscg_fill(counts.data_ptr(), 2 * counts.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
    elif not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == nb):
        raise _lib.SscgError("boundary_counts: counts must be a contiguous int64 [3 C + C C] tensor on the device")
    n, h, w = lt.shape
    check(lib.sscg_boundary_counts(lt.data_ptr(), lp.data_ptr(), n, h, w, c, d, counts.data_ptr(), _stream()), "sscg_boundary_counts")
    return counts


# Surface distances of the evaluation (sscg_surface_stats, include/sscg.h holds the definitions): opt-in (`--surface`).
class SurfaceOptions(object):
    """The two parameters of the surface distances: `tol`, the tolerance of the normalised surface Dice in pixels (finite, >= 0; a
    surface pixel is within it when d <= tol, i.e. d^2 <= floor(tol^2) for the integer d^2), and `pct`, the percentile of HD95 (an
    integer in 1..100; 100 makes it the Hausdorff distance)."""
    __slots__ = ("tol", "pct")

    def __init__(self, tol=2.0, pct=95):
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0.0 <= float(tol) < float("inf"):
            raise ValueError("surface tol %r is not a finite number >= 0" % (tol,))
        if isinstance(pct, bool) or not isinstance(pct, int) or not 1 <= pct <= 100:
            raise ValueError("surface pct %r is not an integer in 1..100" % (pct,))
        self.tol, self.pct = float(tol), pct

    @property
    def tol2(self):
        """floor(tol^2), capped at the largest d^2 an image the kernel accepts can hold."""
        return int(min(math.floor(self.tol * self.tol), 2 ** 30))

    def __eq__(self, other):
        return isinstance(other, SurfaceOptions) and (self.tol, self.pct) == (other.tol, other.pct)

    def __repr__(self):
        return "SurfaceOptions(tol=%r, pct=%r)" % (self.tol, self.pct)


_SURFACE_WS_BYTES = {}


def surface_stats(label_true, label_pred, num_classes, options, *, stats=None, sums=None):
    """The per-case records of the surface distances of a batch (sscg_surface_stats): label_true [N,H,W] (any integer type, values
    outside [0, C) belong to no class), label_pred [N,H,W] class ids as bytes.  Returns (stats int64 [2,N,C,5] = cnt, within, max2,
    v_lo, v_hi per direction (0: true -> predicted), sample and class; sums float64 [2,N,C]) on the device, overwritten.  `stats`,
    `sums`: tensors to use instead of new ones."""
    if not (label_true.is_cuda and label_pred.is_cuda):
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
    if not isinstance(options, SurfaceOptions):
        raise TypeError("options must be a functional.SurfaceOptions, not %r" % (options,))
    c = int(num_classes)
    if label_true.dim() != 3 or tuple(label_true.shape) != tuple(label_pred.shape):
        raise _lib.SscgError("surface_stats: two [N, H, W] label maps of one shape expected, got %s and %s" % (
            tuple(label_true.shape), tuple(label_pred.shape)))
    lt = label_true.to(torch.int64).contiguous()
    lp = label_pred.to(torch.uint8).contiguous()
    n, h, w = lt.shape
    if stats is None:
        stats = torch.empty((2, n, c, 5), dtype=torch.int64, device=lt.device)
    elif not (stats.is_cuda and stats.dtype == torch.int64 and stats.is_contiguous() and tuple(stats.shape) == (2, n, c, 5)):
        raise _lib.SscgError("surface_stats: stats must be a contiguous int64 [2, N, C, 5] tensor on the device")
    if sums is None:
        sums = torch.empty((2, n, c), dtype=torch.float64, device=lt.device)
    elif not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and tuple(sums.shape) == (2, n, c)):
        raise _lib.SscgError("surface_stats: sums must be a contiguous float64 [2, N, C] tensor on the device")
    key = (n, h, w, c)
    if key not in _SURFACE_WS_BYTES:
        _SURFACE_WS_BYTES[key] = lib.sscg_surface_workspace(*key)
    ws = _WS.get(_SURFACE_WS_BYTES[key], lt.device)
    check(lib.sscg_surface_stats(lt.data_ptr(), lp.data_ptr(), n, h, w, c, options.tol2, options.pct, stats.data_ptr(), sums.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream()), "sscg_surface_stats")
    return stats, sums


# Calibration scores of the evaluation (sscg_calib_stats, include/sscg.h holds the definitions): opt-in (`--calibration`).
CALIBRATION_MAX_BINS = 32
CALIBRATION_MAX_TEMPS = 8


class CalibrationOptions(object):
    """The two parameters of the calibration scores: `bins`, the number of equal-width confidence bins of the reliability diagram (an
    integer in 2..32; 15 is the customary count), and `temps`, the temperatures T the softmax is also evaluated at (logits / T) - finite
    numbers > 0, at most 8 with the leading 1.0.  temps[0] is always 1.0, the network as it is: a list that does not start with it gets
    it put in front, and a second 1.0 is dropped.  More than one temperature asks for the fit of the NLL-optimal one."""
    __slots__ = ("bins", "temps")

    def __init__(self, bins=15, temps=(1.0,)):
        if isinstance(bins, bool) or not isinstance(bins, int) or not 2 <= bins <= CALIBRATION_MAX_BINS:
            raise ValueError("calibration bins %r is not an integer in 2..%d" % (bins, CALIBRATION_MAX_BINS))
        if isinstance(temps, (int, float)) and not isinstance(temps, bool):
            temps = (temps,)
        try:
            given = tuple(temps)
        except TypeError:
            raise ValueError("calibration temps %r is not a list of numbers" % (temps,))
        out = [1.0]
        for t in given:
            if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 < float(t) < float("inf"):
                raise ValueError("calibration temperature %r is not a finite number > 0" % (t,))
            t = float(t)
            inv = _inv_temp(t)
            if not 0.0 < inv < float("inf"):
                raise ValueError("calibration temperature %r: 1 / T is not a finite fp32 number > 0" % (t,))
            if t == 1.0:
                continue
            if t in out:
                raise ValueError("calibration temperature %r is given twice" % (t,))
            out.append(t)
        if len(out) > CALIBRATION_MAX_TEMPS:
            raise ValueError("calibration: %d temperatures with the leading 1.0, at most %d" % (len(out), CALIBRATION_MAX_TEMPS))
        self.bins, self.temps = bins, tuple(out)

    @property
    def inv_temps(self):
        """numpy.float32(1) / numpy.float32(T) per temperature: the factors the kernel multiplies the resized logits by."""
        return [_inv_temp(t) for t in self.temps]

    def __eq__(self, other):
        return isinstance(other, CalibrationOptions) and (self.bins, self.temps) == (other.bins, other.temps)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((self.bins, self.temps))

    def __repr__(self):
        return "CalibrationOptions(bins=%r, temps=%r)" % (self.bins, self.temps)


def _inv_temp(t):
    import numpy as np
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        return float(np.float32(1) / np.float32(t))


_CALIB_WS_BYTES = {}


def calibration_stats(x, size, label_true, options, *, probs=False, scale=1.0, state=None):
    """The counts behind the calibration scores of a batch (sscg_calib_stats), accumulated into `state` = (bins int64 [NT,B,3], cls int64
    [NT,C,3], sums float64 [NT,2]) on the device (None = new zeroed ones), which is returned.  `x`: fp32 [N,C,H,W] logits, resized to
    `size` like predict_labels' - their softmax at every temperature of `options` is scored; or, with probs=True, non-negative scores
    already at `size` whose probability is x * scale (prob_sum of predict_labels_ms with scale = 1 / views; q of crf_labels or a
    softmax map with scale = 1) - one temperature only.  `label_true`: N*OH*OW integer labels; values outside [0, C) are not counted."""
    if not isinstance(options, CalibrationOptions):
        raise TypeError("options must be a functional.CalibrationOptions, not %r" % (options,))
    _need_hip(x, f32_only=True)
    if not label_true.is_cuda:
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % label_true.device)
    if x.dim() != 4:
        raise _lib.SscgError("calibration_stats: 4-D logits or scores expected")
    _no_grad_input(x, "calibration_stats")
    xs = to_nhwc(x.detach())
    n, c, h, w = xs.shape
    oh, ow = int(size[0]), int(size[1])
    nt, b = len(options.temps), options.bins
    if probs and (h, w) != (oh, ow):
        raise _lib.SscgError("calibration_stats: scores (probs=True) must already have the output size")
    if probs and nt != 1:
        raise ValueError("calibration_stats: scores (probs=True) have no logits to rescale: one temperature only, got %r" % (options.temps,))
    lt = label_true.to(torch.int64).contiguous()
    if lt.numel() != n * oh * ow:
        raise _lib.SscgError("calibration_stats: label_true must have N*OH*OW elements")
    if state is None:
        flat = torch.empty((nt * (b + c) * 3 + nt * 2,), dtype=torch.int64, device=xs.device)
        check(lib.sscg_fill(flat.data_ptr(), 2 * flat.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per 8-byte zero
        state = (flat[:nt * b * 3].view(nt, b, 3), flat[nt * b * 3:nt * (b + c) * 3].view(nt, c, 3),
                 flat[nt * (b + c) * 3:].view(torch.float64).view(nt, 2))
    bins, cls, sums = state
    for t, dt, shape, what in ((bins, torch.int64, (nt, b, 3), "bins must be a contiguous int64 [NT, B, 3]"),
                               (cls, torch.int64, (nt, c, 3), "cls must be a contiguous int64 [NT, C, 3]"),
                               (sums, torch.float64, (nt, 2), "sums must be a contiguous float64 [NT, 2]")):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise _lib.SscgError("calibration_stats: %s tensor on the device" % what)
    key = (n, oh, ow, nt)
    if key not in _CALIB_WS_BYTES:
        _CALIB_WS_BYTES[key] = lib.sscg_calib_workspace(*key)
    ws = _WS.get(_CALIB_WS_BYTES[key], xs.device)
    its = (C.c_float * nt)(*options.inv_temps)
    check(lib.sscg_calib_stats(xs.data_ptr(), 1 if probs else 0, float(scale), n, h, w, c, oh, ow, lt.data_ptr(), its, nt, b,
                               bins.data_ptr(), cls.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sscg_calib_stats")
    return state


# Connected-component filtering of predicted label maps (sscg_components_filter, include/sscg.h holds the definitions): opt-in
# (`--components`).
class ComponentOptions(object):
    """What the component filter keeps: `largest` = only the largest component of each (sample, class), ties to the one that starts
    first in row-major order; `min_area` = only components of at least that many pixels (0 = no threshold); both may be set.  `conn` =
    4 or 8 (pixel connectivity), `fill` = the class a removed component becomes, `skip` = class ids that are never filtered (the fill
    class never is)."""
    __slots__ = ("largest", "min_area", "conn", "fill", "skip")

    def __init__(self, largest=False, min_area=0, conn=8, fill=0, skip=()):
        if not isinstance(largest, (bool, int)) or largest not in (0, 1):
            raise ValueError("components largest %r is not a bool" % (largest,))
        if isinstance(min_area, bool) or not isinstance(min_area, int) or not 0 <= min_area < 2 ** 31:
            raise ValueError("components min_area %r is not an integer in 0..2^31-1" % (min_area,))
        if isinstance(conn, bool) or conn not in (4, 8):
            raise ValueError("components conn %r is not 4 or 8" % (conn,))
        if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill < 64:
            raise ValueError("components fill %r is not a class id in 0..63" % (fill,))
        try:
            skip = tuple(sorted(set(skip)))
        except TypeError:
            raise ValueError("components skip %r is not a list of class ids" % (skip,))
        if any(isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 64 for s in skip):
            raise ValueError("components skip %r holds something that is not a class id in 0..63" % (skip,))
        self.largest, self.min_area, self.conn, self.fill, self.skip = bool(largest), min_area, conn, fill, skip

    def exempt_mask(self, num_classes):
        """Bit c set = class c is never filtered: the skip list and the fill class, checked against the class count."""
        c = int(num_classes)
        if not 1 <= c <= 64:
            raise ValueError("components: %d classes, 1..64 expected" % c)
        if self.fill >= c:
            raise ValueError("components fill=%d is not a class of %d" % (self.fill, c))
        if any(s >= c for s in self.skip):
            raise ValueError("components skip=%s names a class that is not one of %d" % (":".join(str(s) for s in self.skip), c))
        mask = 1 << self.fill
        for s in self.skip:
            mask |= 1 << s
        return mask

    def _key(self):
        return (self.largest, self.min_area, self.conn, self.fill, self.skip)

    def __eq__(self, other):
        return isinstance(other, ComponentOptions) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "ComponentOptions(largest=%r, min_area=%r, conn=%r, fill=%r, skip=%r)" % self._key()


_COMPONENTS_WS_BYTES = {}


def component_filter(label_pred, num_classes, options, *, label_true=None, hist=None, out=None, stats=False):
    """The component filter on a batch of predicted label maps (sscg_components_filter): label_pred [N,H,W] class ids as bytes.
    Returns (label_u8 uint8 [N,H,W], hist or None, stats or None).  `label_true` ([N,H,W], any integer type; values outside [0, C) are
    void) adds the FILTERED maps to the confusion matrix `hist` (int64 [C,C] on the device, accumulated; None = a new zeroed one);
    `out`: a uint8 [N,H,W] tensor to write instead of a new one (label_pred itself = in place); `stats`: True = a new int64 [N,C,4]
    tensor (components, kept components, pixels before, pixels after per sample and class), or such a tensor, overwritten."""
    if not label_pred.is_cuda or (label_true is not None and not label_true.is_cuda):
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % (
            label_pred.device if not label_pred.is_cuda else label_true.device))
    if not isinstance(options, ComponentOptions):
        raise TypeError("options must be a functional.ComponentOptions, not %r" % (options,))
    c = int(num_classes)
    try:
        mask = options.exempt_mask(c)
    except ValueError as e:
        raise _lib.SscgError("component_filter: %s" % e)
    if label_pred.dim() != 3:
        raise _lib.SscgError("component_filter: an [N, H, W] label map expected, got %s" % (tuple(label_pred.shape),))
    if hist is not None and label_true is None:
        raise _lib.SscgError("component_filter: a confusion matrix needs label_true")
    lp = label_pred.to(torch.uint8).contiguous()
    n, h, w = lp.shape
    lt = None
    if label_true is not None:
        lt = label_true.to(torch.int64).contiguous()
        if lt.numel() != lp.numel():
            raise _lib.SscgError("component_filter: label_true must have N*H*W elements")
        if hist is None:
            hist = torch.empty((c, c), dtype=torch.int64, device=lp.device)
            check(lib.sscg_fill(hist.data_ptr(), 2 * hist.numel(), 0.0, _stream()), "sscg_fill")   # 2 fp32 zeros per int64 zero
        elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == c * c):
            raise _lib.SscgError("component_filter: hist must be a contiguous int64 [C, C] tensor on the device")
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.uint8, device=lp.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, h, w)):
        raise _lib.SscgError("component_filter: out must be a contiguous uint8 [N, H, W] tensor on the device")
    if stats is True:
        stats = torch.empty((n, c, 4), dtype=torch.int64, device=lp.device)
    elif stats is False or stats is None:
        stats = None
    elif not (stats.is_cuda and stats.dtype == torch.int64 and stats.is_contiguous() and tuple(stats.shape) == (n, c, 4)):
        raise _lib.SscgError("component_filter: stats must be a contiguous int64 [N, C, 4] tensor on the device")
    key = (n, h, w, c)
    if key not in _COMPONENTS_WS_BYTES:
        _COMPONENTS_WS_BYTES[key] = lib.sscg_components_workspace(*key)
    ws = _WS.get(_COMPONENTS_WS_BYTES[key], lp.device)
    check(lib.sscg_components_filter(lp.data_ptr(), _ptr(lt), n, h, w, c, options.conn, int(options.largest), options.min_area,
                                     options.fill, mask, out.data_ptr(), _ptr(hist), _ptr(stats), ws.data_ptr(), ws.numel(), _stream()),
          "sscg_components_filter")
    return out, hist, stats


# The per-epoch image panels (sscg_panel_labels / sscg_panel_range / sscg_panel_grid): the grids train() hands to the image writer,
# built on the device.  SSCG_FUSE_PANELS=0 keeps model.panels() on the chain of separate passes and the host (an A/B aid: the bytes
# are the same).
FUSE_PANELS = [os.environ.get("SSCG_FUSE_PANELS", "1") != "0"]
PANEL_IMAGE, PANEL_COLOUR, PANEL_GREY = _lib.PANEL_IMAGE, _lib.PANEL_COLOUR, _lib.PANEL_GREY


def panel_labels(logits, size, want_onehot=True):
    """interp(size) -> Softmax2d -> .max(1)[1] -> make_one_hot of fp32 logits [N,C,H,W] in one launch (model.py:580-585, :593-597).
    Returns (label_u8 uint8 [N,OH,OW], onehot fp32 [N,C,OH,OW] channels-last or None): the ids predict_labels gives, and what
    label_onehot makes of them - neither the resized logits, the probabilities nor an int64 map are written."""
    _need_hip(logits, f32_only=True)
    if logits.dim() != 4:
        raise _lib.SscgError("panel_labels: 4-D logits expected")
    _no_grad_input(logits, "panel_labels")
    x = to_nhwc(logits.detach())
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    u8 = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device)
    onehot = empty_nhwc(n, c, oh, ow, x.device) if want_onehot else None
    check(lib.sscg_panel_labels(x.data_ptr(), n, h, w, c, oh, ow, u8.data_ptr(), _ptr(onehot), _stream()), "sscg_panel_labels")
    return u8, onehot


def _panel_source(src, kind, palette, what):
    """(contiguous source, N, H, W, C) of a panel: IMAGE fp32 [N,C,H,W] (C in {1, 3}; NHWC memory), COLOUR uint8 ids [N,H,W], GREY
    int64 ids [N,H,W] or [N,1,H,W]."""
    if not src.is_cuda:
        raise _lib.SscgError("sscg kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % src.device)
    if kind == PANEL_IMAGE:
        _need_hip(src, f32_only=True)
        if src.dim() != 4 or src.shape[1] not in (1, 3):
            raise _lib.SscgError("%s: an image panel is fp32 [N,C,H,W] with C in {1, 3}" % what)
        _no_grad_input(src, what)
        x = to_nhwc(src.detach())
        n, c, h, w = x.shape
        return x, n, h, w, c
    if kind not in (PANEL_COLOUR, PANEL_GREY):
        raise _lib.SscgError("%s: unknown panel kind %r" % (what, kind))
    want = torch.uint8 if kind == PANEL_COLOUR else torch.int64
    if src.dtype != want:
        raise _lib.SscgError("%s: %s ids expected, got %s" % (what, want, src.dtype))
    if src.dim() == 4 and src.shape[1] == 1:
        src = src.reshape(src.shape[0], src.shape[2], src.shape[3])
    if src.dim() != 3:
        raise _lib.SscgError("%s: ids of shape [N,H,W] expected" % what)
    if kind == PANEL_COLOUR and (palette is None or not palette.is_cuda or palette.dtype != torch.uint8 or palette.numel() != 768
                                 or not palette.is_contiguous()):
        raise _lib.SscgError("%s: a colour panel needs a contiguous uint8 [256,3] palette on the MI355X" % what)
    n, h, w = src.shape
    return src.contiguous(), n, h, w, 1


def panel_range(src, kind, scale=1.0, shift=0.0, palette=None):
    """fp32 [2] on the device: the minimum and maximum of a panel's values (IMAGE: x * scale + shift; COLOUR: the palette's channels
    of every id; GREY: the ids), over the whole batch - make_grid(normalize=True)'s range (model.py:634-638).  No host sync."""
    x, n, h, w, c = _panel_source(src, kind, palette, "panel_range")
    rng = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = _WS.get(lib.sscg_panel_range_workspace(n * h * w, c), x.device)
    check(lib.sscg_panel_range(x.data_ptr(), kind, n * h * w, c, float(scale), float(shift), _ptr(palette), rng.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream()), "sscg_panel_range")
    return rng


def panel_grid_shape(n, h, w, nrow, padding):
    """[3, GH, GW] of torchvision.utils.make_grid for n tiles of h x w"""
    if n == 1:
        return (3, h, w)
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return (3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding)


def panel_grid(src, kind, rng, nrow=8, padding=2, scale=1.0, shift=0.0, palette=None):
    """torchvision.utils.make_grid(t, nrow, padding, normalize=True) + the image writer's (t * 255).astype(uint8) in one launch:
    uint8 [3,GH,GW] on the device.  `rng`: panel_range's result for the same source, scale and shift."""
    x, n, h, w, c = _panel_source(src, kind, palette, "panel_grid")
    if not (rng.is_cuda and rng.dtype == torch.float32 and rng.numel() == 2 and rng.is_contiguous()):
        raise _lib.SscgError("panel_grid: the range is a contiguous fp32 [2] tensor on the MI355X (panel_range)")
    grid = torch.empty(panel_grid_shape(n, h, w, int(nrow), int(padding)), dtype=torch.uint8, device=x.device)
    check(lib.sscg_panel_grid(x.data_ptr(), kind, n, h, w, c, float(scale), float(shift), _ptr(palette), rng.data_ptr(), int(nrow),
                              int(padding), grid.data_ptr(), _stream()), "sscg_panel_grid")
    return grid


def image_u8_to_f32(img_u8, mean, std):
    """uint8 [B,H,W,C] (HWC pixels as PIL decoded them) -> fp32 logical [B,C,H,W], channels-last, ((u/255) - mean) / std:
    ToTensor + Normalize of data_utils/__init__.py:126-150 on the device."""
    if not img_u8.is_cuda or img_u8.dtype != torch.uint8 or img_u8.dim() != 4:
        raise _lib.SscgError("image_u8_to_f32: uint8 [B,H,W,C] tensor on the MI355X expected")
    b, h, w, c = img_u8.shape
    src = img_u8.contiguous()
    dst = torch.empty((b, h, w, c), dtype=torch.float32, device=src.device)
    check(lib.sscg_image_u8_to_f32(src.data_ptr(), dst.data_ptr(), b * h * w, c, mean.data_ptr(), std.data_ptr(), _stream()),
          "sscg_image_u8_to_f32")
    return dst.permute(0, 3, 1, 2)


def label_lut(gt_u8, lut):
    """uint8 label ids [B,H,W] -> int64 [B,1,H,W] through a 256-entry table (ToLabel + Relabel / encode_segmap)."""
    if not gt_u8.is_cuda or gt_u8.dtype != torch.uint8 or lut.dtype != torch.int64 or lut.numel() != 256:
        raise _lib.SscgError("label_lut: uint8 labels on the MI355X and an int64 table of 256 entries expected")
    src = gt_u8.contiguous()
    dst = torch.empty(src.shape, dtype=torch.int64, device=src.device)
    check(lib.sscg_label_lut(src.data_ptr(), dst.data_ptr(), src.numel(), lut.data_ptr(), _stream()), "sscg_label_lut")
    return dst.unsqueeze(1)


def augment_batch(img_u8, gt_u8, mats, out_size, mean, std, lut, image_fill=0, label_fill=0, colour=None, need_mean=False, elastic=None,
                  mix=None):
    """Batched affine augmentation fused into the batch finish (sscg_augment_u8, one launch): uint8 [N,H,W,C] pixels, uint8 [N,H,W]
    label ids (or None) and one int32 Q16 map per sample (`mats` [N,6], data_utils.augmentations.to_q16) -> what image_u8_to_f32 and
    label_lut return for the warped batch: fp32 logical [N,C,OH,OW] channels-last, int64 [N,1,OH,OW] (or None).  Outside the source:
    `image_fill` per tap, the raw id `label_fill` through the table.  Identity maps reproduce the two passes bit for bit.
    `colour` (fp32 [N,21] on the device, data_utils.augmentations.Compose.colours; C of 1 or 3): the samples' colour maps, applied to
    the warped pixels inside the same launch (sscg_augment_colour_u8); `need_mean`: the maps use the image mean (a contrast op), which
    costs a sum pass in front of the launch.  None = the plain entry, as before.
    `elastic` = (nodes, grid): int32 [N,GH,GW,2] control nodes on the device (data_utils.augmentations.Compose.fields) and their
    spacing in output pixels, GH = (OH-1)//grid + 4, GW likewise - a cubic B-spline displacement added to every pixel's source
    coordinate inside the same launch (sscg_augment_elastic_u8), with or without `colour`.  None = the affine entries, as before.
    `mix` = (table, classes): int32 [N,8] on the device (data_utils.augmentations.Compose.mixes: partner, box, class mask per sample)
    and whether the class rule applies (it needs labels) - mixed-sample augmentation, CutMix and ClassMix, decided per output pixel
    inside the same launch (sscg_augment_mix_u8; C of 1 or 3), with whatever of `colour` and `elastic` is given.  None = the entries
    above, as before."""
    if not img_u8.is_cuda or img_u8.dtype != torch.uint8 or img_u8.dim() != 4:
        raise _lib.SscgError("augment_batch: uint8 [N,H,W,C] tensor on the MI355X expected")
    n, h, w, c = img_u8.shape
    if not mats.is_cuda or mats.dtype != torch.int32 or tuple(mats.shape) != (n, 6):
        raise _lib.SscgError("augment_batch: int32 [N,6] matrices on the MI355X expected")
    if gt_u8 is not None and (not gt_u8.is_cuda or gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (n, h, w)
                              or lut is None or lut.dtype != torch.int64 or lut.numel() != 256):
        raise _lib.SscgError("augment_batch: uint8 [N,H,W] labels on the MI355X and an int64 table of 256 entries expected")
    if colour is not None and (not colour.is_cuda or colour.dtype != torch.float32 or tuple(colour.shape) != (n, 21)):
        raise _lib.SscgError("augment_batch: fp32 [N,21] colour table on the MI355X expected")
    oh, ow = int(out_size[0]), int(out_size[1])
    if elastic is not None:
        nodes, grid = elastic[0], int(elastic[1])
        if grid < 4 or oh <= 0 or ow <= 0:
            raise _lib.SscgError("augment_batch: an elastic node spacing of at least 4 output pixels and a positive output size expected")
        gh, gw = (oh - 1) // grid + 4, (ow - 1) // grid + 4
        if not torch.is_tensor(nodes) or not nodes.is_cuda or nodes.dtype != torch.int32 or tuple(nodes.shape) != (n, gh, gw, 2):
            raise _lib.SscgError("augment_batch: int32 [N,%d,%d,2] elastic nodes on the MI355X expected" % (gh, gw))
    if mix is not None:
        mix_table, classes = mix[0], int(bool(mix[1]))
        if not torch.is_tensor(mix_table) or not mix_table.is_cuda or mix_table.dtype != torch.int32 or tuple(mix_table.shape) != (n, 8):
            raise _lib.SscgError("augment_batch: int32 [N,8] mix table on the MI355X expected")
    src, m = img_u8.contiguous(), mats.contiguous()
    dst = torch.empty((n, oh, ow, c), dtype=torch.float32, device=src.device)
    gsrc = gt_u8.contiguous() if gt_u8 is not None else None
    gdst = torch.empty((n, oh, ow), dtype=torch.int64, device=src.device) if gt_u8 is not None else None
    args = (src.data_ptr(), gsrc.data_ptr() if gsrc is not None else None, m.data_ptr(), dst.data_ptr(),
            gdst.data_ptr() if gdst is not None else None, n, h, w, c, oh, ow, mean.data_ptr(), std.data_ptr(),
            lut.data_ptr() if gsrc is not None else None, int(image_fill), int(label_fill))
    if mix is not None:
        table = colour.contiguous() if colour is not None else None
        ws = _WS.get(lib.sscg_augment_colour_workspace(n), src.device) if colour is not None and need_mean else None
        lattice, geom = (nodes.contiguous(), (grid, gh, gw)) if elastic is not None else (None, (0, 0, 0))
        rows = mix_table.contiguous()
        check(lib.sscg_augment_mix_u8(*args, _ptr(table), int(bool(need_mean)), _ptr(ws), _ptr(lattice), *geom, rows.data_ptr(), classes,
                                      _stream()), "sscg_augment_mix_u8")
    elif elastic is not None:
        table = colour.contiguous() if colour is not None else None
        ws = _WS.get(lib.sscg_augment_colour_workspace(n), src.device) if colour is not None and need_mean else None
        lattice = nodes.contiguous()
        check(lib.sscg_augment_elastic_u8(*args, _ptr(table), int(bool(need_mean)), _ptr(ws), lattice.data_ptr(), grid, gh, gw, _stream()),
              "sscg_augment_elastic_u8")
    elif colour is None:
        check(lib.sscg_augment_u8(*args, _stream()), "sscg_augment_u8")
    else:
        table = colour.contiguous()
        ws = _WS.get(lib.sscg_augment_colour_workspace(n), src.device) if need_mean else None
        check(lib.sscg_augment_colour_u8(*args, table.data_ptr(), int(bool(need_mean)), _ptr(ws), _stream()), "sscg_augment_colour_u8")
    return dst.permute(0, 3, 1, 2), (gdst.unsqueeze(1) if gdst is not None else None)


def label_onehot(labels, num_classes):
    """utils.make_one_hot (utils.py:314-350): labels int64 [N,1,H,W] -> fp32 one-hot [N,C,H,W] (NHWC memory)."""
    if not labels.is_cuda or labels.dtype != torch.int64:
        raise _lib.SscgError("int64 HIP label tensor expected")
    labels = labels.contiguous()
    n, _, h, w = labels.shape
    oh = empty_nhwc(n, num_classes, h, w, labels.device)
    check(lib.sscg_label_onehot(labels.data_ptr(), oh.data_ptr(), n * h * w, num_classes, _stream()), "sscg_label_onehot")
    return oh


def _scalar(device):
    return torch.empty((), dtype=torch.float32, device=device)


def _loss_ws(device):
    return _WS.get(lib.sscg_loss_workspace(0), device)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, shadow_bf16=None, shadow_split=None):
    """shadow_bf16: bf16 arena rewritten with the parameters; shadow_split: the 3-plane split arena (3 * numel bf16) instead."""
    sh, sdt = (shadow_split, BF16X3) if shadow_split is not None else (shadow_bf16, BF16)
    check(lib.sscg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(sh), sdt, p.numel(), lr, beta1, beta2,
                             eps, step, grad_scale, _stream()), "sscg_adam_step")


def grad_norm(g, max_norm, grad_scale=1.0, norm=None, clip=None):
    """Global L2 norm of the flat fp32 gradient `g` times grad_scale and clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)),
    both 0-dim device tensors (written into `norm` / `clip` when given): two launches, fp64 fixed-order sums, no host round trip."""
    if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
        raise _lib.SscgError("grad_norm: contiguous fp32 tensor on the MI355X expected")
    norm = _scalar(g.device) if norm is None else norm
    clip = _scalar(g.device) if clip is None else clip
    ws = _WS.get(lib.sscg_grad_norm_workspace(g.numel()), g.device)
    check(lib.sscg_grad_norm(g.data_ptr(), g.numel(), grad_scale, max_norm, norm.data_ptr(), clip.data_ptr(), ws.data_ptr(), ws.numel(),
                             _stream()), "sscg_grad_norm")
    return norm, clip


def adam_step_ex(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, shadow_bf16=None, shadow_split=None, clip=None,
                 weight_decay=0.0, decoupled=False, ema=None, ema_decay=0.0):
    """adam_step with the optimiser options: `clip` a 0-dim device coefficient (grad_norm), weight decay as torch.optim.Adam's L2 term
    or decoupled (torch.optim.AdamW), `ema` an fp32 arena updated as ema.lerp_(p, 1 - ema_decay) in the same launch."""
    sh, sdt = (shadow_split, BF16X3) if shadow_split is not None else (shadow_bf16, BF16)
    check(lib.sscg_adam_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(sh), sdt, _ptr(ema), p.numel(), lr, beta1,
                                beta2, eps, step, grad_scale, _ptr(clip), weight_decay, 1 if decoupled else 0, ema_decay, _stream()),
          "sscg_adam_step_ex")


# ----------------------------------------------------------------------------- autograd functions
_WEIGHT_EPOCH = [0]     # weights owned by no arena optimiser (stock torch optimisers rewrite `_version` instead)


def bump_weight_epoch(epoch_cell=None):
    """Called by the optimiser after it rewrote parameters: invalidates the cached transposed copies of ITS weights
    (`epoch_cell` is the one-element list its parameters carry as `_sscg_epoch`; the discriminators' update must not
    make the generators rebuild 450 transposes)."""
    (epoch_cell if epoch_cell is not None else _WEIGHT_EPOCH)[0] += 1


_WT_USERS = {}      # id -> (weakref of the weight, set of operand-copy kinds a pass has asked for: "t32", "t16", "w16")


def _note_user(w, kind):
    ent = _WT_USERS.get(id(w))
    if ent is None:
        key = id(w)
        ent = _WT_USERS[key] = (weakref.ref(w, lambda _r, key=key: _WT_USERS.pop(key, None)), set())
    ent[1].add(kind)


def refresh_transposed_weights(weights=(), all_users=True):
    """Bring the cached operand copies (transposed fp32 / transposed bf16 / plain bf16) of `weights` - and, with
    `all_users`, of every weight a pass has asked for - up to date on the CURRENT stream.  The step calls this before it
    forks its forward passes over two streams: their backward passes then only read the cache (a lazily rebuilt copy would
    be written on one stream and read on the other).

    `all_users` is only safe on a stream that is ordered behind EVERY optimiser's last update and every reader of the
    stale copies (a rebuild frees the old copy: the allocator may hand its block to the next allocation at once)."""
    _IN_REFRESH[0] = True
    try:
        _refresh_all(weights, all_users)
    finally:
        _IN_REFRESH[0] = False


def _refresh_all(weights, all_users):
    bf16 = _MODE[0] == "bf16"
    jobs = []
    if _MODE[0] != "f32s":       # (split mode: which copy a weight needs depends on its geometry - the registry below knows)
        for w in weights:
            kind = "t16" if (bf16 and w.shape[0] % 64 == 0) else "t32"
            _note_user(w, kind)
            if not all_users:
                _refresh_kinds(w, (kind,), jobs)
    if not all_users:
        if _MODE[0] == "f32s":
            for w in weights:
                ent = _WT_USERS.get(id(w))
                if ent is not None:
                    _refresh_kinds(w, ent[1], jobs)
        _transpose_batch(jobs)
        return
    for r, kinds in list(_WT_USERS.values()):
        w = r()
        if w is None:
            continue
        _refresh_kinds(w, kinds, jobs)
    _transpose_batch(jobs)


_WT_ATTR = {"tx3": "_sscg_wtx3", "t16": "_sscg_wt16", "t32": "_sscg_wt"}
BATCH_TRANSPOSES = [os.environ.get("SSCG_BATCH_TRANSPOSES", "1") != "0"]


def _refresh_kinds(w, kinds, jobs=None):
    """Bring the operand copies `kinds` of weight w up to date.  With `jobs` (a list), a stale TRANSPOSED copy is not rebuilt here:
    the weight is appended and `_transpose_batch` rebuilds all of them in one launch."""
    for kind, dtype in (("t32", torch.float32), ("t16", torch.bfloat16), ("tx3", "x3")):
        if kind in kinds:
            if jobs is not None and BATCH_TRANSPOSES[0]:
                ent = getattr(w, _WT_ATTR[kind], None)
                tag = _wtag(w)
                if ent is None or ent.tag != tag:
                    jobs.append((w, kind, ent, tag))
            else:
                _cached_wt(w, dtype)
    if "w16" in kinds:
        weight_bf16(w)
    if "wx3" in kinds:
        weight_split(w)


class _WtJob(C.Structure):          # include/sscg.h: sscg_wt_job
    _fields_ = [("w", C.c_void_p), ("wt", C.c_void_p), ("w_dtype", C.c_int32), ("wt_dtype", C.c_int32),
                ("K", C.c_int32), ("RS", C.c_int32), ("C", C.c_int32), ("block0", C.c_int32)]


_WT_TABLES = {}      # (source, destination) pointers of a batch -> (device table, blocks): the same weights come back every step


def _transpose_batch(jobs):
    """The stale transposed operand copies of a whole step in ONE launch (sscg_weight_krsc_to_crsk_batch; 234 launches of ~6 us at the
    top of a config-2 step otherwise).  A copy that exists is rewritten IN PLACE - `refresh_transposed_weights` runs ordered behind
    every reader of the stale copies, which is also what freeing them (the per-weight path) needs - so the pointers, and with them
    the job table in device memory, are the same from the second step on."""
    assert _IN_REFRESH[0]
    if len(jobs) < 2:
        for w, kind, _, _ in jobs:
            _cached_wt(w, {"t32": torch.float32, "t16": torch.bfloat16, "tx3": "x3"}[kind])
        return
    rows = []
    blocks = 0
    keep = []
    fast = not hasattr(lib, "note_batch")       # (racecheck.py wants every buffer's extent: it sees them in data_ptr())
    cur = _stream()
    for w, kind, ent, tag in jobs:
        src = weight_bf16(w) if kind == "t16" else w
        row = getattr(ent, "row", None) if (fast and ent is not None) else None
        if row is not None and ent.ev is None and row[0] == (tag[2] if src is w else src.data_ptr()):
            rows.append(row + (blocks,))        # same source, same destination as the last time: rewritten in place
            blocks += ent.nblk
            ent.tag, ent.stream = tag, cur
            continue
        k, c, r, s = w.shape
        temp = not src.is_contiguous(memory_format=CL)
        if temp:
            src = src.contiguous(memory_format=CL)
            keep.append(src)
        t = None
        if ent is not None:
            if ent.ev is None and ent.t.device == w.device:
                t = ent.t               # built by a refresh: its readers are the ones our caller is ordered behind
            else:
                ent.retire()            # built lazily (a model's first step): the allocator keeps the block for its readers
        if t is None:
            t = (torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=w.device) if kind == "tx3" else
                 torch.empty((c, k, r, s), dtype=torch.bfloat16 if kind == "t16" else torch.float32, device=w.device, memory_format=CL))
        wt_dtype = {"t32": F32, "t16": BF16, "tx3": BF16X3}[kind]
        row = (src.data_ptr(), t.data_ptr(), _dt(src), wt_dtype, k, r * s, c)
        rows.append(row + (blocks,))
        copy = _Copy.__new__(_Copy)
        copy.tag, copy.t, copy.stream, copy.ev, copy.readers = tag, t, cur, None, None
        copy.nblk = -(-c // 32) * -(-k // 32) * r * s
        copy.row = None if temp else row
        blocks += copy.nblk
        keep.append((w, kind, copy))
    key = tuple(rows)
    tab = _WT_TABLES.get(key)
    if tab is None:
        if len(_WT_TABLES) >= 16:           # (a table may still be in use on another stream)
            torch.cuda.synchronize()
            _WT_TABLES.clear()
        host = (_WtJob * len(rows))(*[_WtJob(*row) for row in rows])
        dev_t = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(jobs[0][0].device)
        torch.cuda.current_stream().synchronize()       # once per table: later steps launch it from whichever lane refreshes
        tab = _WT_TABLES[key] = (dev_t, rows)
    _note_batch(tab)
    check(lib.sscg_weight_krsc_to_crsk_batch(tab[0].data_ptr(), len(rows), blocks, _stream()), "sscg_weight_krsc_to_crsk_batch")
    for item in keep:
        if isinstance(item, tuple):
            w, kind, copy = item
            try:
                setattr(w, _WT_ATTR[kind], copy)
            except AttributeError:
                pass


def _note_batch(tab):
    """racecheck.py sees pointers in argument lists; the batch's buffers sit in a device table - announce them."""
    if _NOTE_BATCH is not None:
        _NOTE_BATCH(tab[0].data_ptr(), [(row[0], row[1]) for row in tab[1]])


_NOTE_BATCH = getattr(lib, "note_batch", None)      # only racecheck.py's handle has it


def _wtag(w):
    return (w._version, getattr(w, "_sscg_epoch", _WEIGHT_EPOCH)[0], w.data_ptr())


_NO_COPY_SYNC = os.environ.get("SSCG_DBG_NO_COPY_SYNC") == "1"      # A/B aid: round 3's behaviour (tests/aids/fuzz_step.py shows the race)
_IN_REFRESH = [False]       # inside refresh_transposed_weights: the CALLER orders the readers (one event for the whole batch)


class _Copy(object):
    """A cached operand copy of a weight.  A copy built inside `refresh_transposed_weights` is ordered by its caller (one event for
    the batch: model._copies_ready).  A copy built LAZILY - by the first pass that needs it, on that pass's stream - carries its own
    event: a reader on another stream waits for it first (once per stream), and every reader stream is announced to the allocator
    (`record_stream`) when the copy is replaced, so that the block is not handed out while a reader is still in flight.  (Round 3
    had neither: at a model's first step - empty registry, nothing prebuilt - the copies were built by whichever of the two forward
    lanes reached a layer first and read by the other unsynchronised; racecheck.py reports exactly these launches.)"""
    __slots__ = ("tag", "t", "ev", "stream", "readers", "row", "nblk")

    def __init__(self, tag, build):
        self.tag = tag
        self.stream = _stream()
        self.t = build()
        self.readers = None
        self.ev = None
        if not _IN_REFRESH[0] and not _NO_COPY_SYNC:
            self.ev = torch.cuda.Event()
            self.ev.record()
            self.readers = set()

    def get(self):
        if self.ev is not None:
            h = _stream()
            if h != self.stream and h not in self.readers:
                torch.cuda.current_stream().wait_event(self.ev)
                self.readers.add(h)
        return self.t

    def retire(self):
        """The copy is about to be dropped: its block must outlive the readers on other streams."""
        if self.readers:
            dev = self.t.device
            for h in self.readers:
                self.t.record_stream(_stream_object(dev, h))


def _cached_copy(w, attr, build):
    tag = _wtag(w)
    ent = getattr(w, attr, None)
    if ent is None or ent.tag != tag:
        if ent is not None:
            ent.retire()
        ent = _Copy(tag, build)
        try:
            setattr(w, attr, ent)
        except AttributeError:
            pass
    return ent.get()


def _cached_wt(w, dtype=torch.float32):
    """Transposed copy of a weight, cached ON the tensor object (dies with it; a recycled address can never
    alias).  Valid while neither torch (`_version`) nor our optimiser (`_WEIGHT_EPOCH`) has rewritten it."""
    kind = "tx3" if dtype == "x3" else ("t16" if dtype == torch.bfloat16 else "t32")
    _note_user(w, kind)
    attr = {"tx3": "_sscg_wtx3", "t16": "_sscg_wt16", "t32": "_sscg_wt"}[kind]
    return _cached_copy(w, attr, lambda: weight_transposed(w, dtype))


def weight_bf16(w):
    """bf16 operand copy of a conv weight, same [K][R][S][C] layout.  A parameter owned by optim.FusedAdam reads the
    optimiser's bf16 shadow arena (rewritten by the Adam kernel itself: no per-step cast); any other weight (the frozen
    nets) gets a cached cast."""
    _note_user(w, "w16")
    opt = getattr(w, "_sscg_opt", None)
    opt = opt() if opt is not None else None
    if opt is not None:
        return opt.shadow_view(w)
    return _cached_copy(w, "_sscg_w16", lambda: cast(w, torch.bfloat16))


def _split3_copy(w):
    n = w.numel()
    t = torch.empty(3 * n, dtype=torch.bfloat16, device=w.device)
    src = w if w.is_contiguous(memory_format=CL) else w.contiguous(memory_format=CL)
    check(lib.sscg_split3(src.data_ptr(), t.data_ptr(), n, n, _stream()), "sscg_split3")
    return t


def weight_split(w):
    """(three-plane bf16 split copy of a conv weight in its own [K][R][S][C] layout, plane stride in elements): the operand of
    the split contraction.  A parameter owned by optim.FusedAdam reads the optimiser's split shadow arena (rewritten by the
    Adam kernel itself); any other weight (the frozen nets) gets a cached copy."""
    _note_user(w, "wx3")
    opt = getattr(w, "_sscg_opt", None)
    opt = opt() if opt is not None else None
    if opt is not None and hasattr(opt, "split_view"):
        return opt.split_view(w)
    return _cached_copy(w, "_sscg_wx3", lambda: _split3_copy(w)), w.numel()


def _acc_target(param):
    """Gradient arena slice of a parameter owned by optim.FusedAdam (None for a stock optimiser)."""
    acc = getattr(param, "_sscg_grad", None)
    if acc is not None:
        param._sscg_touched = True
    return acc


def _running_stats(running_mean, running_var, per_sample):
    """The running statistics that a batch-statistics pass advances: none for a layer without them or with per-sample (InstanceNorm)
    statistics."""
    if running_mean is not None and per_sample is not True:
        return running_mean, running_var
    return None, None


def _conv_stats_fwd(x, w, bias, geom, out_f32, norm, fallback=True):
    """(y, mean, rstd, (g, l, c)): y = conv(x, w) + bias and the batch statistics of the normalisation layer `norm` = (per_sample, eps,
    running_mean, running_var, momentum) that follows it - from the conv's epilogue where one takes them for the geometry, else
    (`fallback`) from a statistics pass over y; without the fallback mean / rstd are then None."""
    stride, pad, dil, pad_mode = geom
    per_sample, eps, rmean, rvar, momentum = norm
    n, _, h, wd = x.shape
    p, q = conv_out_size(h, w.shape[2], stride, pad, dil), conv_out_size(wd, w.shape[3], stride, pad, dil)
    glc = _glc_shape((n, w.shape[0], p, q), per_sample)
    y, mean, rstd = conv2d_fwd_norm(x, w, bias, stride, pad, dil, pad_mode, out_f32, glc, eps, rmean, rvar, momentum)
    if mean is None and fallback:
        mean, rstd = norm_stats(y, per_sample, eps, *_running_stats(rmean, rvar, per_sample), momentum)
    return y, mean, rstd, glc


def _add_into(acc, src_ptr, count):
    check(lib.sscg_add(acc.data_ptr(), src_ptr, acc.data_ptr(), F32, count, _stream()), "sscg_add")


def _arena_add(device, acc, src_ptr, count, ref, keep):
    """acc += `count` fp32 sums at src_ptr (inside the tensor `keep`), queued on the side lane of the parameter `ref` that owns the
    arena slice `acc`: every gradient of a parameter is accumulated on that parameter's lane."""
    run_on_side_stream(device, (keep,), lambda: _add_into(acc, src_ptr, count), lane=getattr(ref, "_sscg_lane", 0), defer=True)


class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d (+ folded nn.ReflectionPad2d, + fused activation when no norm layer follows).

    `norm` = None, or the description of the normalisation layer that follows - (per_sample, eps, running_mean,
    running_var, momentum): the conv's epilogue then also produces that layer's batch statistics (arch/ops.py:40-57 "Conv +
    InstanceNorm / BatchNorm" blocks) and the function returns (y, mean, rstd); mean is None when the fusion does not apply
    to the geometry (the caller falls back to a statistics pass over y).
    `grad` = the grad mode of the caller (inside forward() it is always off)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, pad_mode, act, slope, out_f32, norm, grad):
        x = to_nhwc(x)
        mean = rstd = None
        if norm is not None and act == ACT_NONE:
            y, mean, rstd, _ = _conv_stats_fwd(x, w, bias, (stride, pad, dil, pad_mode), out_f32, norm, fallback=False)
        else:       # (no conv epilogue takes statistics behind an activation)
            y = conv2d_fwd(x, w, bias, stride, pad, dil, pad_mode, act, slope, out_f32)
        ctx.cfg = (stride, pad, dil, pad_mode, act, slope)
        ctx.has_bias = bias is not None
        ctx.wref = w
        ctx.bref = bias
        ctx.counted = _note_use(w, bias) if grad and ctx.needs_input_grad[1] else ()
        ctx.save_for_backward(x, w, y if act != ACT_NONE else None)
        # (mean, rstd) are non-differentiable outputs: left alone, autograd hands backward() two zero-filled tensors for them -
        # 850 fill launches per Cityscapes step
        ctx.set_materialize_grads(False)
        if norm is None:
            return y
        if mean is None:
            return y, None, None
        ctx.mark_non_differentiable(mean, rstd)
        return y, mean, rstd

    @staticmethod
    def backward(ctx, dy, *_unused):
        if dy is None:          # nothing downstream used y
            return (None,) * 12
        x, w, y = ctx.saved_tensors
        stride, pad, dil, pad_mode, act, slope = ctx.cfg
        dy = to_nhwc(dy)
        if act != ACT_NONE:
            dy = act_bwd(dy, y, act, slope)
        dx, dw, db = _conv_backward(dy, x, w, ctx.wref, ctx.bref if ctx.has_bias else None, (stride, pad, dil, pad_mode),
                                    ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], ctx.counted)
        return dx, dw, db, None, None, None, None, None, None, None, None, None


def _conv_backward(dy, x, w, wref, bref, geom, want_x, want_w, want_b, counted):
    """Backward of y = conv(x, w) + bias for the gradient dy of the PRE-activation output: (dx, dw, db).  Weight / bias gradients of
    parameters owned by optim.FusedAdam go straight into its gradient arena on the parameter's side lane (dw, db then None).
    `counted`: the parameters whose use the forward counted (_note_use); their gradient kernels are queued when this returns."""
    stride, pad, dil, pad_mode = geom
    dx = None
    if want_x:
        if pad_mode == PAD_REFLECT:
            raise _lib.SscgError("input gradient through a reflection-padded conv: use ReflectPadFn + pad=0 conv")
        # x is the output of a conv -> norm -> activation unit that left its normalisation context on the tensor (ConvNormActFn):
        # this data gradient IS that unit's upstream gradient, so its epilogue takes the unit's backward sums and the reduction pass
        # over (dz, y) never runs.  The records travel on dx and are only honoured if dx arrives unchanged (`_version`): an
        # accumulation by the autograd engine (a tensor with two consumers) bumps it.
        # A fan-out (SplitFn) in front - a residual block's input feeds conv1 and the shortcut: the gradient the OTHER consumer already
        # left joins in this data gradient's store phase (`_Join`), the result is then the tensor's total gradient (and the sums above
        # apply to it); SplitFn.backward has nothing left to add.
        fuse = FUSE_BSUMS[0] and stride == 1 and x.dtype == dy.dtype and (x.dtype == torch.float32 or FUSE_BSUMS_BF16[0])
        join = getattr(x, "_sscg_join", None) if FUSE_JOIN[0] else None
        addend = None
        if join is not None:
            addend = join[0].take(join[1])
            info = join[0].norm if (fuse and addend is not None) else None
        else:
            info = getattr(x, "_sscg_norm", None) if fuse else None
        if info is not None and len(info) > 8 and info[8] and x.dtype != torch.float32:
            info = None             # (mask read off the unit's output: fp32 tensors only)
        # A ReLU unit's sums are taken with its mask in registers: dx is stored masked (PREMASK) and the unit's apply pass skips the mask
        # and the residual's gradient.  The flag travels with the records; without records dx is the unmasked total as before.
        premask = PREMASK[0] and info is not None and info[6] == ACT_RELU and x.dtype == torch.float32 and dy.dtype == torch.float32
        if info is not None or addend is not None:
            dx, rec, joined = conv2d_dgrad_param(dy, wref, x.shape, w.shape, stride, pad, dil, out_dtype=x.dtype, bsums=info, addend=addend, z=x,
                                                 premask=premask)
            if addend is not None and not joined:
                rec = None          # the sums saw a partial gradient
            if rec is not None:
                dx._sscg_bsums = (rec, dx._version, premask)
            if join is not None:
                if joined:
                    join[0].folded = (join[1], dx)
                else:
                    join[0].deposit(join[1], dx)
        else:
            dx = conv2d_dgrad_param(dy, wref, x.shape, w.shape, stride, pad, dil, out_dtype=x.dtype)
            if join is not None:
                join[0].deposit(join[1], dx)
    dw, db = _param_grads(x, dy, dy, w.shape, geom, wref, bref, want_w, want_b)
    _note_done(counted)
    return dx, dw, db


def _param_grads(a, b, dy, wshape, geom, wref, bref, want_w, want_b):
    """Parameter gradients of a convolution: (dw, db) with dw = wgrad(a, b) (input and output gradient of the conv that is
    differentiated) and db = the column sums of dy.  Gradients of parameters owned by optim.FusedAdam are accumulated straight into
    its gradient arena instead (returned as None), always on the parameter's own side lane (fixed accumulation order)."""
    stride, pad, dil, pad_mode = geom
    dw = db = None
    wacc = _acc_target(wref) if want_w else None
    bacc = _acc_target(bref) if want_b else None
    n, k, p, q = dy.shape

    def arena_grads():
        if wacc is not None:
            conv2d_wgrad(a, b, wshape, stride, pad, dil, pad_mode, out=wacc, accumulate=True)
        if bacc is not None:
            colsum(n * p * q, k, dy, out=bacc, accumulate=True)

    if wacc is not None or bacc is not None:
        # nothing on the backward critical path reads these: run them beside the data-gradient chain
        run_on_side_stream(dy.device, (a, b), arena_grads, lane=getattr(wref, "_sscg_lane", 0), defer=True)
    if want_w and wacc is None:
        dw = conv2d_wgrad(a, b, wshape, stride, pad, dil, pad_mode)
    if want_b and bacc is None:
        db = colsum(n * p * q, k, dy)
    return dw, db


class ConvTranspose2dFn(torch.autograd.Function):
    """nn.ConvTranspose2d (arch/ops.py:55-56) as the data-gradient of the mirrored convolution.

    `w` is the torch ConvTranspose2d weight, logical [Cin, Cout, R, S], channels-last memory
    [Cin][R][S][Cout] - i.e. the [K][R][S][C] weight of a conv Cout->Cin.  Its parameters are not counted for the bucketed
    exchange (GRAD_READY): their bucket goes out after the backward."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, out_pad, act, slope, out_f32=False):
        x = to_nhwc(x)
        n, cin, h, wd = x.shape
        cin2, cout, r, s = w.shape
        oh = (h - 1) * stride - 2 * pad + (r - 1) + out_pad + 1
        ow = (wd - 1) * stride - 2 * pad + (s - 1) + out_pad + 1
        # mirrored conv: input [n, cout, oh, ow] -> output [n, cin, h, wd]
        if conv_out_size(oh, r, stride, pad, 1) != h or conv_out_size(ow, s, stride, pad, 1) != wd:
            raise _lib.SscgError("unsupported ConvTranspose2d geometry")
        # the transposed operand copy [Cout][R][S][Cin] comes from the per-parameter cache inside conv2d_dgrad
        y = conv2d_dgrad_param(x, w, (n, cout, oh, ow), (cin, cout, r, s), stride, pad, 1, bias, act, slope,
                               out_dtype=_out_dtype(out_f32))
        ctx.cfg = (stride, pad, act, slope)
        ctx.has_bias = bias is not None
        ctx.wref, ctx.bref = w, bias
        ctx.save_for_backward(x, w, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, act, slope = ctx.cfg
        dy = to_nhwc(dy)
        if act != ACT_NONE:
            dy = act_bwd(dy, y, act, slope)
        dx = None
        if ctx.needs_input_grad[0]:
            # gradient wrt x = forward of the mirrored conv applied to dy
            dx = conv2d_fwd(dy, w, None, stride, pad, 1, out_f32=(x.dtype == torch.float32))
        # mirrored conv has input dy (as "x") and output-gradient x (as "dy")
        dw, db = _param_grads(dy, x, dy, w.shape, (stride, pad, 1, PAD_ZEROS), ctx.wref, ctx.bref,
                              ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return dx, dw, db, None, None, None, None, None, None


class NormActFn(torch.autograd.Function):
    """InstanceNorm2d / BatchNorm2d (+ residual add) + activation, one statistics pass + one apply pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, per_sample, training, momentum, eps, act, slope,
                pre_mean=None, pre_rstd=None):
        x = to_nhwc(x)
        if residual is not None:
            residual = to_nhwc(residual)
        use_batch_stats = training or running_mean is None
        if use_batch_stats and pre_mean is not None:
            mean, rstd = pre_mean, pre_rstd      # produced by the conv's epilogue (running statistics already advanced there)
        elif use_batch_stats:
            rmean, rvar = _running_stats(running_mean, running_var, per_sample) if training else (None, None)
            mean, rstd = norm_stats(x, per_sample, eps, rmean, rvar, momentum)
        else:
            per_sample = False          # running statistics: one (mean, rstd) row whatever the grouping
            mean = running_mean.view(1, -1)
            rstd = rstd_from_var(running_var, eps).view(1, -1)
        y = norm_apply(x, mean, rstd, gamma, beta, residual, per_sample, act, slope)
        ctx.cfg = (per_sample, act, slope, use_batch_stats, residual is not None)
        ctx.gref, ctx.betaref = gamma, beta
        # y supplies the activation mask of the backward; without a residual (and for ReLU / LeakyReLU) the mask is the sign of
        # gamma * xhat + beta, which the backward kernels recompute from x: one tensor less to read in both of them
        need_y = act != ACT_NONE and (residual is not None or act not in (ACT_RELU, ACT_LRELU))
        ctx.save_for_backward(x, y if need_y else None, mean, rstd, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, gamma, beta = ctx.saved_tensors
        per_sample, act, slope, stats_grad, has_res = ctx.cfg
        dx, ret_g, ret_b, dres = _norm_backward(to_nhwc(dy), x, y, mean, rstd, gamma, beta, ctx.gref, ctx.betaref, per_sample, act, slope,
                                                stats_grad, gamma is not None and ctx.needs_input_grad[1],
                                                has_res and ctx.needs_input_grad[3])
        if not ctx.needs_input_grad[0]:
            dx = None
        return dx, ret_g, ret_b, dres, None, None, None, None, None, None, None, None, None, None


def _norm_backward(dy, x, y, mean, rstd, gamma, beta, gref, betaref, per_sample, act, slope, stats_grad, want_g, want_dres):
    """Backward of y = act(norm(x) [+ residual]): (dx, dgamma, dbeta, dres).  dgamma / dbeta of parameters owned by optim.FusedAdam are
    added into its gradient arena on the parameter's side lane (returned as None)."""
    dgamma = dbeta = dgb = None
    ret_g = ret_b = None
    gacc = bacc = None
    rec = getattr(dy, "_sscg_bsums", None)
    from_sums = (rec is not None and rec[1] == dy._version and stats_grad and act in (ACT_NONE, ACT_RELU, ACT_LRELU)
                 and (y is not None) == bool(rec[0][2]))        # (the sums' mask source: the unit's output iff a residual joined an activated unit)
    if want_g:
        gacc = _acc_target(gref)
        bacc = _acc_target(betaref)
        fin = rec[0][3] if (from_sums and len(rec[0]) > 3) else None
        if fin is not None:     # dgamma / dbeta were written by the data gradient's call, behind the coefficients
            dgb = fin[fin.numel() - 2 * gamma.numel():].view(2, gamma.numel())
        else:
            dgb = torch.empty((2, gamma.numel()), dtype=torch.float32, device=gamma.device)     # written (not accumulated) by the kernel: no zero fill
        dgamma, dbeta = dgb[0], dgb[1]
        if gacc is None or bacc is None:
            gacc = bacc = None
            ret_g, ret_b = dgamma, dbeta
    if from_sums and len(rec) > 2 and rec[2] and act == ACT_RELU:
        # dy arrived masked (a ReLU unit; the data gradient that took the sums stored gg): the apply pass has no mask to form, and the
        # residual's gradient is dy itself - no tensor allocated, nothing written.  The records are spent: the alias travels on.
        dy._sscg_bsums = None
        dx, _ = norm_bwd_from_sums(rec[0], dy, x, mean, rstd, gamma, beta, per_sample, ACT_NONE, 0.0, dgamma, dbeta)
        dres = dy if want_dres else None
    elif from_sums:
        dx, dres = norm_bwd_from_sums(rec[0], dy, x, mean, rstd, gamma, beta, per_sample, act, slope, dgamma, dbeta, y=y, want_dres=want_dres)
    else:
        dx, dres = norm_bwd(dy, x, y, mean, rstd, gamma, per_sample, act, slope, stats_grad,
                            want_dres=want_dres, dgamma=dgamma, dbeta=dbeta, beta=beta, overwrite=True)
    if gacc is not None:
        # The sums were produced beside dx on this stream; their accumulation into the optimiser's arena runs on the
        # parameter's own side lane, like every other gradient of that parameter (two forward lanes may both reach
        # this layer: a read-modify-write of the arena slice from two streams would lose updates).  weight and bias of a
        # norm layer are neighbours in the arena: one launch adds both.
        n_c = gacc.numel()
        if bacc.data_ptr() == gacc.data_ptr() + 4 * n_c:
            _arena_add(dy.device, gacc, dgb.data_ptr(), 2 * n_c, gref, dgb)
        else:       # (one deferred call on gamma's lane for the pair, as the adjacent case)
            def both():
                _add_into(gacc, dgamma.data_ptr(), n_c)
                _add_into(bacc, dbeta.data_ptr(), n_c)
            run_on_side_stream(dy.device, (dgb,), both, lane=getattr(gref, "_sscg_lane", 0), defer=True)
    return dx, ret_g, ret_b, dres


class ConvNormActFn(torch.autograd.Function):
    """The reference's fusion unit as ONE autograd node: conv -> InstanceNorm / BatchNorm (batch statistics, from the conv's
    epilogue where the library can fuse them) [+ residual] -> activation (arch/ops.py:40-57; Bottleneck conv+bn pairs,
    arch/generators.py:345-365).  The same kernels as Conv2dFn + NormActFn; one node instead of two halves the host's per-layer
    autograd cost (575 such pairs per step).  cfg = (stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, grad);
    grad = the grad mode of the caller (inside forward() it is always off)."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, residual, running_mean, running_var, cfg):
        stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, grad = cfg
        x = to_nhwc(x)
        if residual is not None:
            residual = to_nhwc(residual)
        y, mean, rstd, glc = _conv_stats_fwd(x, w, bias, (stride, pad, dil, pad_mode), False,
                                             (per_sample, eps, running_mean, running_var, momentum))
        z = norm_apply(y, mean, rstd, gamma, beta, residual, per_sample, act, slope)
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.wref, ctx.bref, ctx.gref, ctx.betaref = w, bias, gamma, beta
        ctx.counted = _note_use(w, bias) if grad and ctx.needs_input_grad[1] else ()
        need_z = act != ACT_NONE and (residual is not None or act not in (ACT_RELU, ACT_LRELU))
        ctx.save_for_backward(x, w, y, z if need_z else None, mean, rstd, gamma, beta)
        ctx.res_join = getattr(residual, "_sscg_join", None) if (residual is not None and FUSE_JOIN[0]) else None
        # (only for a forward that will see a backward: the attribute keeps y, mean, rstd alive as long as z lives - the frozen
        # generators, evaluation and validation would hold every pre-norm activation for nothing)
        if (FUSE_BSUMS[0] and grad and any(ctx.needs_input_grad) and act in (ACT_NONE, ACT_RELU, ACT_LRELU)
                and (residual is None or FUSE_JOIN[0])):
            # for the consumer's data gradient (_conv_backward): what this unit's backward reduction needs besides dz; last entry: the
            # mask cannot be recomputed from y (a residual joined before the activation) - it is read off z, the consumer's own input
            z._sscg_norm = (y, mean, rstd, gamma, beta, glc, act, slope, need_z)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w, y, z, mean, rstd, gamma, beta = ctx.saved_tensors
        stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, _ = ctx.cfg
        ni = ctx.needs_input_grad
        dy, ret_g, ret_b, dres = _norm_backward(to_nhwc(dz), y, z, mean, rstd, gamma, beta, ctx.gref, ctx.betaref, per_sample, act, slope,
                                                True, gamma is not None and ni[3], ctx.has_res and ni[5])
        if ctx.res_join is not None and dres is not None:
            ctx.res_join[0].deposit(ctx.res_join[1], dres)      # the shortcut's gradient: the block's conv1 may add it in its data gradient
        dx, dw, db = _conv_backward(dy, x, w, ctx.wref, ctx.bref if ctx.has_bias else None, (stride, pad, dil, pad_mode),
                                    ni[0], ni[1], ctx.has_bias and ni[2], ctx.counted)
        return dx, dw, db, ret_g, ret_b, dres, None, None, None


def _head_fwd(y, mean, rstd, gamma, beta, hw, hbias, per_sample, act, slope):
    """(out, hw32): the fused tail norm -> activation -> Conv2d(c, 1, 1x1) over the pre-norm map y (sscg_norm_head_fwd: the head's
    output is formed while normalising) and the head's weight as the flat fp32 vector its kernels read."""
    hw32 = hw.detach().reshape(-1)
    if hw32.dtype != torch.float32:
        hw32 = hw32.float()
    return norm_head_fwd(y, mean, rstd, gamma, beta, hw32, hbias, per_sample, act, slope), hw32


def _head_backward(dout, y, mean, rstd, gamma, beta, hw32, gref, betaref, hwref, hbref, per_sample, act, slope, want_g, want_hw, want_hb):
    """Backward of _head_fwd: (dy, dgamma, dbeta, dhw, dhbias) with dy the gradient of the pre-norm map (sscg_norm_head_bwd rebuilds
    dout * hw and the activation from y in registers).  The four parameter gradients are sums produced beside dy on this stream; for
    parameters owned by optim.FusedAdam their accumulation into its arena runs on each parameter's own side lane (returned as None)."""
    dout = dout.contiguous()
    if dout.dtype != torch.float32:
        dout = dout.float()
    c = hw32.numel()
    dgb = torch.empty((2, c), dtype=torch.float32, device=y.device) if want_g else None
    dwb = torch.empty(c + 1, dtype=torch.float32, device=y.device)
    dy = norm_head_bwd(dout, hw32, y, mean, rstd, gamma, beta, per_sample, act, slope, True, dwb,
                       dgb[0] if want_g else None, dgb[1] if want_g else None)
    ret_hw = ret_hb = ret_g = ret_b = None
    hwacc = _acc_target(hwref) if want_hw else None
    hbacc = _acc_target(hbref) if want_hb else None
    if want_hw and hwacc is None:
        ret_hw = dwb[:c].reshape(hwref.shape).to(hwref.dtype)
    if want_hb and hbacc is None:
        ret_hb = dwb[c:c + 1].clone()
    gacc = _acc_target(gref) if want_g else None
    bacc = _acc_target(betaref) if want_g else None
    if want_g and (gacc is None or bacc is None):
        gacc = bacc = None
        ret_g, ret_b = dgb[0], dgb[1]
    if hwacc is not None:
        _arena_add(y.device, hwacc, dwb.data_ptr(), c, hwref, dwb)
    if hbacc is not None:
        _arena_add(y.device, hbacc, dwb.data_ptr() + 4 * c, 1, hbref, dwb)
    if gacc is not None:
        _arena_add(y.device, gacc, dgb.data_ptr(), c, gref, dgb)
        _arena_add(y.device, bacc, dgb.data_ptr() + 4 * c, c, betaref, dgb)
    return dy, ret_g, ret_b, ret_hw, ret_hb


class ConvNormActHeadFn(torch.autograd.Function):
    """PixelDiscriminator from its second conv on (arch/discriminators.py:70-75): Conv2d(ndf, 2 ndf, 1x1) -> norm (batch statistics
    from the conv's epilogue) -> LeakyReLU -> Conv2d(2 ndf, 1, 1x1), ONE autograd node.  The 2 ndf-channel map is written once (by
    the conv) and read once per direction of the tail: the head's output is formed while normalising (sscg_norm_head_fwd), and the
    backward rebuilds dy = dout * w3 and the activation from x in registers (sscg_norm_head_bwd) - the normalised map, the head's
    input gradient and the head's weight-gradient pass over it never exist in HBM.
    cfg = (stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, grad); grad = the grad mode of the caller."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, hw, hbias, running_mean, running_var, cfg):
        stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, grad = cfg
        x = to_nhwc(x)
        y, mean, rstd, _ = _conv_stats_fwd(x, w, bias, (stride, pad, dil, pad_mode), False,
                                           (per_sample, eps, running_mean, running_var, momentum))
        out, hw32 = _head_fwd(y, mean, rstd, gamma, beta, hw, hbias, per_sample, act, slope)
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.has_hbias = hbias is not None
        ctx.wref, ctx.bref, ctx.gref, ctx.betaref, ctx.hwref, ctx.hbref = w, bias, gamma, beta, hw, hbias
        ctx.counted = _note_use(w, bias) if grad and ctx.needs_input_grad[1] else ()
        ctx.save_for_backward(x, w, y, mean, rstd, gamma, beta, hw32)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, y, mean, rstd, gamma, beta, hw32 = ctx.saved_tensors
        stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, _ = ctx.cfg
        ni = ctx.needs_input_grad
        dy, ret_g, ret_b, ret_hw, ret_hb = _head_backward(dout, y, mean, rstd, gamma, beta, hw32, ctx.gref, ctx.betaref, ctx.hwref, ctx.hbref,
                                                          per_sample, act, slope, gamma is not None and ni[3], ni[5], ctx.has_hbias and ni[6])
        dx, dw, db = _conv_backward(dy, x, w, ctx.wref, ctx.bref if ctx.has_bias else None, (stride, pad, dil, pad_mode),
                                    ni[0], ni[1], ctx.has_bias and ni[2], ctx.counted)
        return dx, dw, db, ret_g, ret_b, ret_hw, ret_hb, None, None, None


class PixelDiscFn(torch.autograd.Function):
    """The whole PixelDiscriminator (arch/discriminators.py:66-80) as one autograd node: Conv2d(cin, 64, 1x1) -> LeakyReLU ->
    Conv2d(64, 2 ndf, 1x1) [+ the norm layer's batch statistics] in ONE launch (sscg_conv2d_front_fwd: the 64-channel map is formed
    in LDS and written only for a backward pass), then the fused tail of ConvNormActHeadFn (norm -> LeakyReLU -> Conv2d(2 ndf, 1, 1x1)
    while normalising).  The backward is the chain of the separate nodes: head / norm, second conv, LeakyReLU mask, first conv.
    cfg = (slope1, per_sample, eps, momentum, act, slope, grad); grad = the grad mode of the caller."""

    @staticmethod
    def forward(ctx, x, w1, b1, w, bias, gamma, beta, hw, hbias, running_mean, running_var, cfg):
        slope1, per_sample, eps, momentum, act, slope, grad = cfg
        x = to_nhwc(x)
        n, _, h, wd = x.shape
        g, l, c = _glc_shape((n, w.shape[0], h, wd), per_sample)
        will = grad and any(ctx.needs_input_grad)
        y, h1, cs = conv2d_front_fwd(x, w1, b1, slope1, w, bias, (g, l, c), want_h1=will)
        mean, rstd = norm_stats_from_conv(cs, (g, l, c), eps, *_running_stats(running_mean, running_var, per_sample), momentum)
        out, hw32 = _head_fwd(y, mean, rstd, gamma, beta, hw, hbias, per_sample, act, slope)
        ctx.cfg = cfg
        ctx.has_b1, ctx.has_bias, ctx.has_hbias = b1 is not None, bias is not None, hbias is not None
        ctx.w1ref, ctx.b1ref, ctx.wref, ctx.bref, ctx.gref, ctx.betaref, ctx.hwref, ctx.hbref = w1, b1, w, bias, gamma, beta, hw, hbias
        ctx.counted1 = _note_use(w1, b1) if grad and ctx.needs_input_grad[1] else ()
        ctx.counted = _note_use(w, bias) if grad and ctx.needs_input_grad[3] else ()
        if will:
            ctx.save_for_backward(x, w1, h1, w, y, mean, rstd, gamma, beta, hw32)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, h1, w, y, mean, rstd, gamma, beta, hw32 = ctx.saved_tensors
        slope1, per_sample, eps, momentum, act, slope, _ = ctx.cfg
        ni = ctx.needs_input_grad
        dy, ret_g, ret_b, ret_hw, ret_hb = _head_backward(dout, y, mean, rstd, gamma, beta, hw32, ctx.gref, ctx.betaref, ctx.hwref, ctx.hbref,
                                                          per_sample, act, slope, gamma is not None and ni[5], ni[7], ctx.has_hbias and ni[8])
        geom = (1, 0, 1, PAD_ZEROS)
        front = ni[0] or ni[1] or (ctx.has_b1 and ni[2])
        dh1, dw, db = _conv_backward(dy, h1, w, ctx.wref, ctx.bref if ctx.has_bias else None, geom, front, ni[3], ctx.has_bias and ni[4],
                                     ctx.counted)
        dx = dw1 = db1 = None
        if front:
            dh1 = act_bwd(dh1, h1, ACT_LRELU, slope1)
            dx, dw1, db1 = _conv_backward(dh1, x, w1, ctx.w1ref, ctx.b1ref if ctx.has_b1 else None, geom, ni[0], ni[1], ctx.has_b1 and ni[2],
                                          ctx.counted1)
        return dx, dw1, db1, dw, db, ret_g, ret_b, ret_hw, ret_hb, None, None, None


def pixel_disc(x, w1, b1, slope1, w, bias, gamma, beta, hw, hbias, running_mean, running_var, per_sample, eps, momentum, act, slope):
    return PixelDiscFn.apply(x, w1, b1, w, bias, gamma, beta, hw, hbias, running_mean, running_var,
                             (slope1, per_sample, eps, momentum, act, slope, torch.is_grad_enabled()))


def conv_norm_act_head(x, w, bias, stride, pad, dil, pad_mode, gamma, beta, hw, hbias, running_mean, running_var, per_sample, eps,
                       momentum, act, slope):
    """conv -> norm (batch statistics) -> activation -> 1x1 conv to one channel, as one node (PixelDiscriminator's tail)."""
    return ConvNormActHeadFn.apply(x, w, bias, gamma, beta, hw, hbias, running_mean, running_var,
                                   (stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, torch.is_grad_enabled()))


class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        _need_hip(x)
        if not (x.is_contiguous() or x.is_contiguous(memory_format=CL)):
            x = x.contiguous()
        y = act_fwd(x, act, slope)
        ctx.cfg = (act, slope)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        act, slope = ctx.cfg
        if dy.stride() != y.stride():
            dy = to_nhwc(dy) if y.is_contiguous(memory_format=CL) else dy.contiguous()
        return act_bwd(dy, y, act, slope), None, None


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = to_nhwc(a), to_nhwc(b)
        return add(a, b)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


FUSE_JOIN = [os.environ.get("SSCG_FUSE_JOIN", "1") != "0"]       # a fan-out's gradient sum inside the last consumer's data gradient


class _Join(object):
    """The fan-out of one activation over n consumers (SplitFn), seen from their backward passes.  A consumer announces the gradient it
    produced (`deposit`); a later consumer whose data gradient can add a tensor in its store phase takes it (`take`) and marks the
    fan-in as done (`folded`): SplitFn.backward then has nothing left to add.  Only for n == 2, only on the stream the deposit was
    produced on (the engine orders the consumers of one pass; a deposit from another lane would be read unordered)."""
    __slots__ = ("n", "norm", "slots", "streams", "folded", "broken")

    def __init__(self, n, norm):
        self.n, self.norm = n, norm
        self.slots, self.streams = [None] * n, [None] * n
        self.folded, self.broken = None, False

    def take(self, i):
        if self.broken or self.n != 2 or self.folded is not None or self.slots[i] is not None:
            return None
        g = self.slots[1 - i]
        if g is None or self.streams[1 - i] != _stream():
            return None
        return g

    def deposit(self, i, g):
        if self.slots[i] is not None or self.folded is not None:
            self.broken = True          # an alias with two consumers: leave everything to SplitFn.backward
        self.slots[i], self.streams[i] = g, _stream()

    def clear(self):
        self.slots, self.streams = [None] * self.n, [None] * self.n
        self.folded, self.broken = None, False


class SplitFn(torch.autograd.Function):
    """Explicit fan-out of an activation that two (or more) consumers read - a residual block's input, the generated
    image that feeds a generator, a discriminator and the L1 loss.  Forward returns aliases; backward sums the
    consumers' gradients with the HIP add kernel in a fixed order, instead of leaving the accumulation to autograd's
    own (torch) add kernel - unless the last consumer's data gradient already added the other one (`_Join`)."""

    @staticmethod
    def forward(ctx, x, n, join=None):
        ctx.join = join
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        join = ctx.join
        if join is not None and join.folded is not None:
            i, t = join.folded
            g = grads[i]
            if join.broken or g is None or g.data_ptr() != t.data_ptr() or g.shape != t.shape:
                raise _lib.SscgError("fan-in bookkeeping: the folded gradient did not arrive unchanged")
            join.clear()
            return t, None, None        # (t carries the backward sums of the unit in front, if its data gradient took them)
        if join is not None:
            join.clear()
        total = None
        for g in grads:
            if g is None:
                continue
            total = to_nhwc(g) if total is None else add(total, to_nhwc(g))
        return total, None, None


class BatchSplitFn(torch.autograd.Function):
    """k batches stacked along N -> k tensors (views).  Backward stacks the k gradients again (device copies)."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        ctx.shape = x.shape
        return tuple(t for t in x.chunk(k, 0))

    @staticmethod
    def backward(ctx, *grads):
        n = ctx.shape[0] // ctx.k
        ref = next(g for g in grads if g is not None)
        out = torch.empty(ctx.shape, dtype=ref.dtype, device=ref.device).contiguous(memory_format=CL)
        for i, g in enumerate(grads):
            if g is None:
                fill_(out[i * n:(i + 1) * n], 0.0)
            else:
                out[i * n:(i + 1) * n].copy_(g)
        return out, None


def split_batch(x, k):
    x = to_nhwc(x)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return x.chunk(k, 0)
    return BatchSplitFn.apply(x, k)


def split(x, n=2):
    """n aliases of x whose gradients are summed by `sscg_add` (no-op outside a gradient-recording forward).
    CONTRACT: every alias has exactly ONE consumer (that is what the aliases are for: a tensor read by k nodes is split k ways).  With
    n == 2 the second consumer's data gradient may add the first one's gradient in its own store phase (`_Join`); an alias that is read
    twice after all breaks that bookkeeping - `_Join.deposit` notices the second deposit and leaves the sum to SplitFn.backward
    (`broken`), and where the fold has already happened SplitFn.backward raises rather than return a silently wrong sum."""
    if n < 2 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    join = _Join(n, getattr(x, "_sscg_norm", None)) if (FUSE_JOIN[0] and n == 2) else None
    outs = SplitFn.apply(x, n, join)
    if join is not None:
        for i, o in enumerate(outs):
            o._sscg_join = (join, i)
    return outs


class DropoutFn(torch.autograd.Function):
    """nn.Dropout(0.5) in training mode.  The keep-mask is a pure function of (seed, element index)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = to_nhwc(x)
        ctx.cfg = (p, seed)
        return dropout(x, p, seed)

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.cfg
        return dropout(to_nhwc(dy), p, seed), None, None


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = to_nhwc(x)
        y, idx = maxpool_fwd(x)
        ctx.xshape = tuple(x.shape)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        return maxpool_bwd(to_nhwc(dy), idx, ctx.xshape)


class MaxPool2Fn(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) (utils.Vgg16: torchvision VGG16 features[4, 9, 16])."""

    @staticmethod
    def forward(ctx, x):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = empty_nhwc(n, c, h // 2, w // 2, x.device, x.dtype)
        idx = torch.empty((n, h // 2, w // 2, c), dtype=torch.uint8, device=x.device)
        check(lib.sscg_maxpool2x2_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), _dt(x), n, h, w, c, _stream()), "sscg_maxpool2x2_fwd")
        ctx.xshape = (n, c, h, w)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = ctx.xshape
        dx = empty_nhwc(n, c, h, w, dy.device, dy.dtype)
        check(lib.sscg_maxpool2x2_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), _dt(dy), n, h, w, c, _stream()), "sscg_maxpool2x2_bwd")
        return dx


def maxpool2x2(x):
    return MaxPool2Fn.apply(x)


class UpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        x = to_nhwc(x)
        ctx.hw = (x.shape[2], x.shape[3])
        return upsample_fwd(x, oh, ow)

    @staticmethod
    def backward(ctx, dy):
        return upsample_bwd(to_nhwc(dy), *ctx.hw), None, None


class SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = softmax_fwd(to_nhwc(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return softmax_bwd(to_nhwc(dy), y)


def ce_weight(values, num_classes, device):
    """The class-weight operand of the weighted cross entropy: `values` (a sequence of C numbers) checked on the host - length C, every
    entry finite and >= 0 - and sent to `device` as fp32 [C].  The check is made here, once; the loss calls only look at the tensor's
    dtype, device and length (no host sync per step)."""
    import math
    vals = [float(v) for v in values]
    if len(vals) != int(num_classes):
        raise ValueError("class weights: %d entries for %d classes" % (len(vals), num_classes))
    for i, v in enumerate(vals):
        if not math.isfinite(v) or v < 0:
            raise ValueError("class weights: entry %d (%r) is not a finite number >= 0" % (i, v))
    return torch.tensor(vals, dtype=torch.float32).to(device)


def _class_weight_ok(weight, c, device, what):
    """A class-weight operand (what: "class" = the cross entropy's, "dice") is None or what ce_weight / dice_weight make."""
    if weight is not None and not (isinstance(weight, torch.Tensor) and weight.dtype == torch.float32 and weight.device == device
                                   and weight.dim() == 1 and weight.numel() == c and weight.is_contiguous()):
        raise _lib.SscgError("%s weights must be a contiguous fp32 [%d] tensor on %s (functional.%s_weight makes one)"
                             % (what, c, device, "ce" if what == "class" else what))


def _check_labels(labels, count):
    if labels.numel() != count or labels.dtype != torch.int64:
        raise _lib.SscgError("labels must be int64 with N*OH*OW elements (N*H*W without a resize): %d" % count)


def _ce_options(weight, label_smoothing, c, device):
    """(weight tensor or None, smoothing as a float, whether the weighted entries are needed) of a cross-entropy call."""
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError("label_smoothing %r is outside [0, 1)" % (label_smoothing,))
    _class_weight_ok(weight, c, device, "class")
    return weight, eps, weight is not None or eps != 0.0


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss(weight, label_smoothing)(logits [N,C,H,W], labels [N,H,W]) - mean over the counted pixels (the sum of their
    class weights when weighted).  weight: fp32 [C] on the device, or None; label_smoothing: 0.0 for none."""

    @staticmethod
    def forward(ctx, logits, labels, weight, label_smoothing):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        labels = labels.contiguous()
        n, c, h, w = logits.shape
        _check_labels(labels, n * h * w)
        weight, eps, weighted = _ce_options(weight, label_smoothing, c, logits.device)
        loss = _scalar(logits.device)
        valid = _scalar(logits.device)      # pixels with a label in [0, C): the divisor of the mean (all of them in the reference)
        ws = _loss_ws(logits.device)
        if weighted:
            check(lib.sscg_ce_fwd_w(logits.data_ptr(), labels.data_ptr(), n * h * w, c, _ptr(weight), eps, loss.data_ptr(),
                                    valid.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sscg_ce_fwd_w")
        else:
            check(lib.sscg_ce_fwd(logits.data_ptr(), labels.data_ptr(), n * h * w, c, loss.data_ptr(), valid.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream()), "sscg_ce_fwd")
        ctx.ce = (weight, eps, weighted)
        ctx.save_for_backward(logits, labels, valid)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, valid = ctx.saved_tensors
        weight, eps, weighted = ctx.ce
        n, c, h, w = logits.shape
        dx = torch.empty_like(logits, memory_format=CL)
        if weighted:
            check(lib.sscg_ce_bwd_w(logits.data_ptr(), labels.data_ptr(), n * h * w, c, _ptr(weight), eps, g.data_ptr(), 1.0,
                                    valid.data_ptr(), dx.data_ptr(), _stream()), "sscg_ce_bwd_w")
        else:
            check(lib.sscg_ce_bwd(logits.data_ptr(), labels.data_ptr(), n * h * w, c, g.data_ptr(), 1.0, valid.data_ptr(),
                                  dx.data_ptr(), _stream()), "sscg_ce_bwd")
        return dx, None, None, None


FUSE_HEAD = [os.environ.get("SSCG_FUSE_HEAD", "1") != "0"]      # interp -> {softmax, cross entropy} without the resized logits in memory


MAX_CLASSES = 64      # SSCG_MAXC of csrc/head_common.h: the class-axis kernels hold one pixel's classes in registers


def _head_applies(x, oh, ow):
    """One block per source pixel gathers the output pixels around it: worth it when the map grows (DeepLab's 33x33 -> the crop)."""
    return (FUSE_HEAD[0] and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] <= MAX_CLASSES
            and oh * ow >= 16 * x.shape[2] * x.shape[3])


def _label_head_forward(x, oh, ow, labels, want_soft, want_ce, weight, eps):
    """The forward launch of the label head on channels-last x: (softmax map, loss, valid, dl), each None where its branch is off.
    weight / eps: _ce_options' - the weighted entry runs only where there is something weighted to compute."""
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, oh, ow, x.device) if want_soft else None
    loss = valid = dl = ws = None
    if want_ce:
        loss, valid = _scalar(x.device), _scalar(x.device)
        dl = empty_nhwc(n, c, h, w, x.device)
        ws = torch.empty(lib.sscg_upsample_head_workspace(n, h, w), dtype=torch.uint8, device=x.device)
    if want_ce and (weight is not None or eps != 0.0):
        check(lib.sscg_upsample_head_fwd_w(x.data_ptr(), labels.data_ptr(), _ptr(weight), eps, _ptr(y), _ptr(loss), _ptr(valid), _ptr(dl),
                                           n, h, w, c, oh, ow, _ptr(ws), ws.numel(), _stream()), "sscg_upsample_head_fwd_w")
    else:
        check(lib.sscg_upsample_head_fwd(x.data_ptr(), _ptr(labels if want_ce else None), _ptr(y), _ptr(loss), _ptr(valid), _ptr(dl),
                                         n, h, w, c, oh, ow, _ptr(ws), ws.numel() if ws is not None else 0, _stream()),
              "sscg_upsample_head_fwd")
    return y, loss, valid, dl


# ----------------------------------------------------------------------------- soft Dice (opt-in; include/sscg.h: sscg_dice_fwd)
def dice_weight(values, num_classes, device):
    """The class-weight operand of the Dice loss, as ce_weight: `values` (C numbers) checked on the host - length C, every entry finite
    and >= 0, and not all zero (the loss divides by their sum) - and sent to `device` as fp32 [C]."""
    w = ce_weight(values, num_classes, torch.device("cpu"))
    if not float(w.sum()) > 0.0:
        raise ValueError("dice weights: every entry is 0 (the loss divides by their sum)")
    return w.to(device)


class DiceOptions(object):
    """The Dice branch of upsample_softmax_ce_dice: weight (dice_weight's tensor, or None = all ones), smooth (> 0), batch (False: one
    Dice per sample and class, averaged; True: the whole call is one group), ce (False: the cross entropy is not wanted - Dice only)."""
    __slots__ = ("weight", "smooth", "batch", "ce")

    def __init__(self, weight=None, smooth=1.0, batch=False, ce=True):
        self.weight, self.smooth, self.batch, self.ce = weight, float(smooth), bool(batch), bool(ce)


def _dice_options(weight, smooth, batch, c, device):
    s = float(smooth)
    if not (s > 0.0 and s < float("inf")):
        raise ValueError("dice smooth %r is not a finite number > 0" % (smooth,))
    _class_weight_ok(weight, c, device, "dice")
    return weight, s, 1 if batch else 0


def dice_fwd(x, labels, size, weight=None, smooth=1.0, batch=False, want_sums=False):
    """sscg_dice_fwd on channels-last fp32 logits x [N,C,H,W] and int64 labels [N,OH,OW] (size = (OH, OW); (H, W): the flat Dice):
    (loss, coef [G,C,2] = (A, B), sums [G,C,3] fp64 = (I, P, T) or None).  No autograd: dice_loss / upsample_softmax_ce_dice wrap it."""
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    _check_labels(labels, n * oh * ow)
    weight, s, b = _dice_options(weight, smooth, batch, c, x.device)
    groups = 1 if b else n
    loss = _scalar(x.device)
    coef = torch.empty((groups, c, 2), dtype=torch.float32, device=x.device)
    sums = torch.empty((groups, c, 3), dtype=torch.float64, device=x.device) if want_sums else None
    ws = torch.empty(lib.sscg_dice_workspace(n, oh, ow, c), dtype=torch.uint8, device=x.device)
    check(lib.sscg_dice_fwd(x.data_ptr(), labels.data_ptr(), n, h, w, c, oh, ow, _ptr(weight), s, b, loss.data_ptr(), _ptr(sums),
                            coef.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sscg_dice_fwd")
    return loss, coef, sums


class DiceLossFn(torch.autograd.Function):
    """Soft Dice loss of logits [N,C,H,W] against labels [N,H,W] (include/sscg.h: sscg_dice_fwd / sscg_dice_bwd)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, smooth, batch):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        labels = labels.contiguous()
        loss, coef, _ = dice_fwd(logits, labels, logits.shape[2:], weight, smooth, batch)
        ctx.batch = 1 if batch else 0
        ctx.save_for_backward(logits, labels, coef)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, coef = ctx.saved_tensors
        n, c, h, w = logits.shape
        dx = torch.empty_like(logits, memory_format=CL)
        check(lib.sscg_dice_bwd(logits.data_ptr(), labels.data_ptr(), n, h, w, c, coef.data_ptr(), ctx.batch, g.data_ptr(), 1.0,
                                dx.data_ptr(), _stream()), "sscg_dice_bwd")
        return dx, None, None, None, None


def dice_loss(logits, labels, weight=None, smooth=1.0, batch=False):
    """1 - mean over (group, class) of the class-weighted soft Dice of softmax(logits) against labels; labels outside [0, C) are void.
    weight: dice_weight's tensor.  batch=False: one group per sample; True: the whole batch is one group."""
    return DiceLossFn.apply(logits, labels, weight, smooth, batch)


# ----------------------------------------------------------------------------- hard-pixel mining (opt-in; include/sscg.h: sscg_ohem_fwd)
class OhemOptions(object):
    """Online hard example mining of a cross entropy: the loss runs over the counted pixels whose probability of the true class does
    not exceed max(thresh, m), m = the r-th smallest such probability of the call, r = clamp(max(min_kept, ceil(min_frac * V)), 1, V)
    of its V counted pixels.  thresh in (0, 1], min_kept an integer >= 0, min_frac in [0, 1]."""
    __slots__ = ("thresh", "min_kept", "min_frac")

    def __init__(self, thresh, min_kept=0, min_frac=0.0):
        t, f = float(thresh), float(min_frac)
        if not 0.0 < t <= 1.0:
            raise ValueError("ohem thresh %r is outside (0, 1]" % (thresh,))
        if isinstance(min_kept, float) and min_kept != int(min_kept):
            raise ValueError("ohem min_kept %r is not an integer" % (min_kept,))
        k = int(min_kept)
        if k < 0 or k >= 2 ** 63:
            raise ValueError("ohem min_kept %r is not an integer >= 0" % (min_kept,))
        if not 0.0 <= f <= 1.0:
            raise ValueError("ohem min_frac %r is outside [0, 1]" % (min_frac,))
        self.thresh, self.min_kept, self.min_frac = t, k, f


def _ohem_options(ohem):
    if isinstance(ohem, dict):
        ohem = OhemOptions(**ohem)
    if not isinstance(ohem, OhemOptions):
        raise TypeError("ohem must be a functional.OhemOptions (or a dict of its arguments), not %r" % (ohem,))
    return ohem


_OHEM_LAST = [None]


def ohem_stats():
    """(thr, kept, V) of the last mined cross entropy of this process: tau as an fp32 scalar and the two int64 counts, all on the
    device - reading them here costs no sync.  None before the first such call."""
    return _OHEM_LAST[0]


def ohem_fwd(x, labels, size, ohem, weight=None, label_smoothing=0.0):
    """sscg_ohem_fwd on channels-last fp32 logits x [N,C,H,W] and int64 labels [N,OH,OW] (size = (OH, OW); (H, W): the flat form):
    (loss, valid = D, keys fp32 [N,OH,OW], thr, counts int64 [2] = (kept, V)).  No autograd: cross_entropy / upsample_softmax_ce wrap it."""
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    _check_labels(labels, n * oh * ow)
    ohem = _ohem_options(ohem)
    weight, eps, _ = _ce_options(weight, label_smoothing, c, x.device)
    loss, valid, thr = _scalar(x.device), _scalar(x.device), _scalar(x.device)
    keys = torch.empty((n, oh, ow), dtype=torch.float32, device=x.device)
    counts = torch.empty((2,), dtype=torch.int64, device=x.device)
    ws = torch.empty(lib.sscg_ohem_workspace(n, oh, ow), dtype=torch.uint8, device=x.device)
    check(lib.sscg_ohem_fwd(x.data_ptr(), labels.data_ptr(), n, h, w, c, oh, ow, _ptr(weight), eps, ohem.thresh, ohem.min_kept,
                            ohem.min_frac, keys.data_ptr(), loss.data_ptr(), valid.data_ptr(), thr.data_ptr(), counts.data_ptr(),
                            ws.data_ptr(), ws.numel(), _stream()), "sscg_ohem_fwd")
    _OHEM_LAST[0] = (thr, counts[0], counts[1])
    return loss, valid, keys, thr, counts


class OhemCrossEntropyFn(torch.autograd.Function):
    """CrossEntropyFn over the mined pixels of logits [N,C,H,W] (include/sscg.h: sscg_ohem_fwd / sscg_ce_bwd_ohem)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, label_smoothing, ohem):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        labels = labels.contiguous()
        loss, valid, keys, thr, _ = ohem_fwd(logits, labels, logits.shape[2:], ohem, weight, label_smoothing)
        ctx.ce = (weight, float(label_smoothing))
        ctx.save_for_backward(logits, labels, keys, thr, valid)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, keys, thr, valid = ctx.saved_tensors
        weight, eps = ctx.ce
        n, c, h, w = logits.shape
        dx = torch.empty_like(logits, memory_format=CL)
        check(lib.sscg_ce_bwd_ohem(logits.data_ptr(), labels.data_ptr(), keys.data_ptr(), thr.data_ptr(), n * h * w, c, _ptr(weight), eps,
                                   g.data_ptr(), 1.0, valid.data_ptr(), dx.data_ptr(), _stream()), "sscg_ce_bwd_ohem")
        return dx, None, None, None, None


# ----------------------------------------------------------------------------- boundary loss (opt-in; include/sscg.h: sscg_sdm)
def boundary_weight(values, num_classes, device):
    """The class-weight operand of the boundary loss, as dice_weight: C numbers, finite, >= 0, not all zero (the loss divides by
    their sum), sent to `device` as fp32 [C]."""
    w = ce_weight(values, num_classes, torch.device("cpu"))
    if not float(w.sum()) > 0.0:
        raise ValueError("boundary weights: every entry is 0 (the loss divides by their sum)")
    return w.to(device)


class BoundaryLossOptions(object):
    """The boundary branch of upsample_softmax_losses: weight (boundary_weight's tensor, or None = all ones)."""
    __slots__ = ("weight",)

    def __init__(self, weight=None):
        self.weight = weight


def _boundary_options(boundary):
    if isinstance(boundary, dict):
        boundary = BoundaryLossOptions(**boundary)
    if not isinstance(boundary, BoundaryLossOptions):
        raise TypeError("boundary must be a functional.BoundaryLossOptions (or a dict of its arguments), not %r" % (boundary,))
    return boundary


def signed_distance_maps(labels, num_classes):
    """sscg_sdm: int64 labels [N,H,W] on the device -> int32 [N,H,W,C], per class +d2 outside it and -d2 inside, d2 = the exact squared
    Euclidean distance to the nearest pixel of the opposite membership in the sample; a class absent from a sample (or filling it)
    has a zero plane.  Labels outside [0, C) belong to no class."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64 and labels.dim() == 3):
        raise _lib.SscgError("signed_distance_maps: labels must be an int64 [N, H, W] tensor on the GPU")
    labels = labels.contiguous()
    n, h, w = labels.shape
    c = int(num_classes)
    sdm = torch.empty((n, h, w, c), dtype=torch.int32, device=labels.device)
    ws = torch.empty(lib.sscg_sdm_workspace(n, h, w, c), dtype=torch.uint8, device=labels.device)
    check(lib.sscg_sdm(labels.data_ptr(), n, h, w, c, sdm.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sscg_sdm")
    return sdm


def boundary_loss_fwd(x, labels, size, sdm, weight=None, want_sums=False):
    """sscg_boundary_loss_fwd on channels-last fp32 logits x [N,C,H,W], int64 labels [N,OH,OW] and their signed_distance_maps
    (size = (OH, OW); (H, W): the flat form): (loss, coef = k, sums [N,C] fp64 or None, counted int64 scalar or None).  No autograd."""
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    _check_labels(labels, n * oh * ow)
    _class_weight_ok(weight, c, x.device, "boundary")
    if sdm.dtype != torch.int32 or sdm.numel() != n * oh * ow * c or not sdm.is_contiguous() or sdm.device != x.device:
        raise _lib.SscgError("sdm must be a contiguous int32 [N, OH, OW, C] tensor on %s (functional.signed_distance_maps makes one)" % x.device)
    loss, coef = _scalar(x.device), _scalar(x.device)
    sums = torch.empty((n, c), dtype=torch.float64, device=x.device) if want_sums else None
    counted = torch.empty((), dtype=torch.int64, device=x.device) if want_sums else None
    ws = torch.empty(lib.sscg_boundary_loss_workspace(n, oh, ow, c), dtype=torch.uint8, device=x.device)
    check(lib.sscg_boundary_loss_fwd(x.data_ptr(), labels.data_ptr(), sdm.data_ptr(), n, h, w, c, oh, ow, _ptr(weight), loss.data_ptr(),
                                     _ptr(sums), _ptr(counted), coef.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "sscg_boundary_loss_fwd")
    return loss, coef, sums, counted


class BoundaryLossFn(torch.autograd.Function):
    """Boundary loss of logits [N,C,H,W] against labels [N,H,W] (include/sscg.h: sscg_sdm, sscg_boundary_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, labels, weight):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        labels = labels.contiguous()
        sdm = signed_distance_maps(labels, logits.shape[1])
        loss, coef, _, _ = boundary_loss_fwd(logits, labels, logits.shape[2:], sdm, weight)
        ctx.weight = weight
        ctx.save_for_backward(logits, labels, sdm, coef)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, sdm, coef = ctx.saved_tensors
        n, c, h, w = logits.shape
        dx = torch.empty_like(logits, memory_format=CL)
        check(lib.sscg_boundary_loss_bwd(logits.data_ptr(), labels.data_ptr(), sdm.data_ptr(), n, h, w, c, _ptr(ctx.weight), coef.data_ptr(),
                                         g.data_ptr(), 1.0, dx.data_ptr(), _stream()), "sscg_boundary_loss_bwd")
        return dx, None, None


def boundary_loss(logits, labels, weight=None):
    """Kervadec's boundary loss: the mean over the counted pixels of sum_c w_c softmax(logits)_c phi_c / sum_c w_c, phi the level set
    of the labels' signed distance maps (signed_distance_maps; computed here, on the device).  It may be negative.  weight:
    boundary_weight's tensor."""
    return BoundaryLossFn.apply(logits, labels, weight)


# ----------------------------------------------------------------------------- Lovasz-softmax (opt-in; include/sscg.h: sscg_lovasz_fwd)
def sort_u32_desc(keys, upper=None):
    """sscg_sort_u32_desc: the rows of `keys` ([S, L] or [L]; int32 or uint32 on the device, read as unsigned 32-bit words) in
    descending order and, int32, the position each key had in its row - equal keys keep ascending position.  upper: every key is
    below it (None: no bound), which lets the sort skip the passes over digits that are zero in every key."""
    if not (isinstance(keys, torch.Tensor) and keys.is_cuda and keys.dtype in (torch.int32, torch.uint32) and keys.dim() in (1, 2)):
        raise _lib.SscgError("sort_u32_desc: keys must be an int32 / uint32 [S, L] or [L] tensor on the GPU")
    keys = keys.contiguous()
    s, l = (1, keys.shape[0]) if keys.dim() == 1 else keys.shape
    up = 0 if upper is None else int(upper)
    if not 0 <= up < 2 ** 32:
        raise ValueError("sort_u32_desc: upper %r is outside [0, 2^32)" % (upper,))
    out = torch.empty_like(keys)
    index = torch.empty(keys.shape, dtype=torch.int32, device=keys.device)
    if keys.numel() == 0:
        return out, index
    ws = torch.empty(lib.sscg_sort_ws_bytes(s, l), dtype=torch.uint8, device=keys.device)
    check(lib.sscg_sort_u32_desc(keys.data_ptr(), s, l, up, out.data_ptr(), index.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "sscg_sort_u32_desc")
    return out, index


class LovaszOptions(object):
    """The Lovasz-softmax loss (include/sscg.h: sscg_lovasz_fwd): classes ("present": the mean runs over the classes with a
    foreground pixel in the segment; "all": over every class), per_image (False: the call is one segment; True: one per sample, the
    mean over the samples with a counted pixel), skip (class ids that never take part, under either setting of `classes`)."""
    __slots__ = ("classes", "per_image", "skip")

    def __init__(self, classes="present", per_image=False, skip=()):
        if classes not in ("present", "all"):
            raise ValueError("lovasz classes %r is neither 'present' nor 'all'" % (classes,))
        ids = []
        for v in skip:
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < MAX_CLASSES:
                raise ValueError("lovasz skip: %r is not a class id in [0, %d)" % (v, MAX_CLASSES))
            if v in ids:
                raise ValueError("lovasz skip: class %d is listed twice" % v)
            ids.append(v)
        self.classes, self.per_image, self.skip = classes, bool(per_image), tuple(sorted(ids))

    def skip_mask(self, c):
        """The skip list as the entry's bit mask, checked against the class count."""
        mask = 0
        for v in self.skip:
            if v >= c:
                raise ValueError("lovasz skip: class %d of %d classes" % (v, c))
            mask |= 1 << v
        if self.classes == "all" and mask == (1 << c) - 1:
            raise ValueError("lovasz: classes='all' with every class skipped leaves nothing to average")
        return mask


def _lovasz_options(lovasz):
    if lovasz is None:
        return LovaszOptions()
    if isinstance(lovasz, dict):
        lovasz = LovaszOptions(**lovasz)
    if not isinstance(lovasz, LovaszOptions):
        raise TypeError("lovasz must be a functional.LovaszOptions (or a dict of its arguments), not %r" % (lovasz,))
    return lovasz


def lovasz_fwd(x, labels, size, lovasz=None, want_class=False):
    """sscg_lovasz_fwd on channels-last fp32 logits x [N,C,H,W] and int64 labels [N,OH,OW] (size = (OH, OW); (H, W): the flat form):
    (loss, coef fp32 [N,OH,OW,C] = d loss / d softmax, keys int32 [segments,C,pixels] = bits(e) + 1, per-class losses [C] or None).
    No autograd: lovasz_softmax / upsample_softmax_losses wrap it."""
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    _check_labels(labels, n * oh * ow)
    lovasz = _lovasz_options(lovasz)
    mask = lovasz.skip_mask(c)
    per_image = 1 if lovasz.per_image else 0
    nws = lib.sscg_lovasz_workspace(n, oh, ow, c, per_image)
    if nws == 0:
        raise _lib.SscgError("lovasz: N * C * OH * OW = %d is not below 2^31" % (n * c * oh * ow))
    segs = n if per_image else 1
    keys = torch.empty((segs, c, n * oh * ow // segs), dtype=torch.int32, device=x.device)
    coef = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    loss = _scalar(x.device)
    per_class = torch.empty((c,), dtype=torch.float32, device=x.device) if want_class else None
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    check(lib.sscg_lovasz_fwd(x.data_ptr(), labels.data_ptr(), n, h, w, c, oh, ow, 1 if lovasz.classes == "all" else 0, per_image, mask,
                              keys.data_ptr(), coef.data_ptr(), loss.data_ptr(), _ptr(per_class), ws.data_ptr(), ws.numel(), _stream()),
          "sscg_lovasz_fwd")
    return loss, coef, keys, per_class


def _lovasz_upstream(coef, g, dy):
    """g * coef [+ dy]: the upstream gradient of the softmax map the backward entries receive, channels-last [N,C,OH,OW]."""
    n, oh, ow, c = coef.shape
    out = empty_nhwc(n, c, oh, ow, coef.device)
    check(lib.sscg_lovasz_scale_add(coef.data_ptr(), g.data_ptr(), _ptr(dy), out.data_ptr(), coef.numel(), _stream()),
          "sscg_lovasz_scale_add")
    return out


class LovaszSoftmaxFn(torch.autograd.Function):
    """Lovasz-softmax loss of logits [N,C,H,W] against labels [N,H,W], the flat form (include/sscg.h: sscg_lovasz_fwd): the forward
    leaves d loss / d softmax, the backward is sscg_softmax_bwd on it."""

    @staticmethod
    def forward(ctx, logits, labels, lovasz):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        labels = labels.contiguous()
        loss, coef, _, _ = lovasz_fwd(logits, labels, logits.shape[2:], lovasz)
        ctx.save_for_backward(logits, coef)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, coef = ctx.saved_tensors
        return softmax_bwd(_lovasz_upstream(coef, g.contiguous(), None), softmax_fwd(logits)), None, None


def lovasz_softmax(logits, labels, lovasz=None):
    """The Lovasz-softmax loss (Berman et al., CVPR 2018) of softmax(logits) against labels; labels outside [0, C) are void.
    lovasz: a LovaszOptions (or a dict of its arguments; None = the defaults)."""
    return LovaszSoftmaxFn.apply(logits, labels, _lovasz_options(lovasz))


# ----------------------------------------------------------------------------- the fused label head: one node for every option
class LabelHeadFn(torch.autograd.Function):
    """interp (bilinear, align_corners=True) -> softmax2d and / or the losses, from the LOW-resolution logits (model.py:390-392, 398,
    401-402, 455): returns (softmax map or None, cross entropy or None, Dice loss or None); the resized logits never reach memory.
    weight / eps: the class-weighted, smoothed cross entropy (None / 0.0: plain); dice: a DiceOptions or None; ohem: an OhemOptions
    (the cross entropy runs over the mined pixels) or None.  Forward: the head's own launch where the softmax map or an unmined cross
    entropy is wanted - that cross entropy's gradient depends on logits and labels only, so the launch already leaves it (dl, up to
    g / valid: `valid` is the sum of the counted pixels' class weights) - then sscg_ohem_fwd (keys, selection, loss) and the Dice
    statistics with their finish.  The selection and the Dice sums couple the pixels of the call, so those two leave no gradient.
    boundary: a BoundaryLossOptions or None - given, the node returns a fourth value, the boundary loss (sscg_sdm on the labels, then
    sscg_boundary_loss_fwd), and every live branch of its backward rides in sscg_upsample_head_bwd_b; not given, the node is the one
    it always was, three values included.
    lovasz: a LovaszOptions or None - given, the node returns one more value, the last: the Lovasz-softmax loss (sscg_lovasz_fwd, which
    leaves d loss / d softmax as a coefficient map).  Its backward is no branch of the stencil: g * coef is added to the upstream
    gradient of the softmax map (sscg_lovasz_scale_add) and whichever entry the other live branches select carries it.
    Backward: ONE launch for every live branch."""

    @staticmethod
    def forward(ctx, x, oh, ow, labels, want_soft, want_ce, weight, eps, dice, ohem, boundary=None, lovasz=None):
        _need_hip(x, f32_only=True)
        x = to_nhwc(x)
        n, c = x.shape[:2]
        if labels is not None:
            labels = labels.contiguous()
            _check_labels(labels, n * oh * ow)
        weight, eps, _ = _ce_options(weight, eps, c, x.device)
        mined = want_ce and ohem is not None
        plain_ce = want_ce and not mined
        y = loss = valid = dl = keys = thr = d_loss = coef = b_loss = sdm = b_coef = None
        if want_soft or plain_ce or not (mined or dice is not None or boundary is not None or lovasz is not None):      # (nothing wanted at all: the entry refuses the call)
            y, loss, valid, dl = _label_head_forward(x, oh, ow, labels, want_soft, plain_ce, weight, eps)
        if mined:
            loss, valid, keys, thr, _ = ohem_fwd(x, labels, (oh, ow), ohem, weight, eps)
        if dice is not None:
            d_loss, coef, _ = dice_fwd(x, labels, (oh, ow), dice.weight, dice.smooth, dice.batch)
        ctx.opts = (oh, ow, weight, eps, 1 if dice is not None and dice.batch else 0)
        # the Lovasz branch: its loss is one more value at the end, its coefficient map one more saved tensor at the end
        ctx.lovasz = lovasz is not None
        ctx.nin = 10 + (1 if boundary is not None or ctx.lovasz else 0) + (1 if ctx.lovasz else 0)
        l_out = l_saved = ()
        if ctx.lovasz:
            l_loss, l_coef, _, _ = lovasz_fwd(x, labels, (oh, ow), lovasz)
            l_out, l_saved = (l_loss,), (l_coef,)
        if boundary is not None:
            sdm = signed_distance_maps(labels.view(n, oh, ow), c)
            b_loss, b_coef, _, _ = boundary_loss_fwd(x, labels, (oh, ow), sdm, boundary.weight)
            # the boundary backward forms the unmined cross entropy in its stencil: the gradient the forward launch left is not kept
            ctx.boundary = (boundary.weight, want_ce)
            ctx.save_for_backward(x, labels, valid, coef, keys, thr, sdm, b_coef, *l_saved)
            ctx.set_materialize_grads(False)
            return (y, loss, d_loss, b_loss) + l_out
        ctx.boundary = None
        # only what a live branch reads: the labels just where a mined or Dice branch gathers by them
        ctx.save_for_backward(x, *((labels,) if mined or dice is not None else ()), dl, valid, coef, keys, thr, *l_saved)
        # an output nothing differentiates (the step reads lab_gt's softmax through .detach() only): backward gets None, not a
        # zero-filled [B, C, crop] map to gather over
        ctx.set_materialize_grads(False)
        return (y, loss, d_loss) + l_out

    @staticmethod
    def backward(ctx, dy, g_ce, g_dice, *g_rest):
        saved = ctx.saved_tensors
        if ctx.lovasz:
            # g_lovasz * coef joins (or is) the upstream gradient of the softmax map: the entries below see one more live dy_soft
            g_lov, g_rest, l_coef, saved = g_rest[-1], g_rest[:-1], saved[-1], saved[:-1]
            if g_lov is not None:
                dy = _lovasz_upstream(l_coef, g_lov.contiguous(), to_nhwc(dy) if dy is not None else None)
        if ctx.boundary is not None:
            return LabelHeadFn._backward_b(ctx, saved, dy, g_ce, g_dice, g_rest[0] if g_rest else None)
        x, labels = saved[0], (saved[1] if len(saved) == 7 else None)
        dl, valid, coef, keys, thr = saved[-5:]
        oh, ow, weight, eps, batch = ctx.opts
        mined = g_ce is not None and keys is not None          # a loss that received no gradient took no part in what was differentiated
        use_ce = g_ce is not None and dl is not None
        use_dice = g_dice is not None and coef is not None
        if dy is None and not (mined or use_ce or use_dice):
            return (None,) * ctx.nin
        n, c, h, w = x.shape
        dx = empty_nhwc(n, c, h, w, x.device)
        if dy is not None:
            dy = to_nhwc(dy)
        ce = (_ptr(dl if use_ce else None), _ptr(g_ce if use_ce else None), _ptr(valid if use_ce else None))
        dice = (_ptr(coef if use_dice else None), _ptr(g_dice if use_dice else None), batch)
        if mined:
            check(lib.sscg_upsample_head_bwd_h(x.data_ptr(), labels.data_ptr(), keys.data_ptr(), thr.data_ptr(), _ptr(weight), eps, _ptr(dy),
                                               g_ce.data_ptr(), valid.data_ptr(), dice[0], dice[1], dice[2], dx.data_ptr(), n, h, w, c, oh, ow,
                                               _stream()), "sscg_upsample_head_bwd_h")
        elif use_dice:
            check(lib.sscg_upsample_head_bwd_d(x.data_ptr(), labels.data_ptr(), _ptr(dy), ce[0], ce[1], ce[2], dice[0], dice[1], dice[2],
                                               dx.data_ptr(), n, h, w, c, oh, ow, _stream()), "sscg_upsample_head_bwd_d")
        else:       # (dy None: the cross entropy alone - the entry scales dl)
            check(lib.sscg_upsample_head_bwd(x.data_ptr(), _ptr(dy), ce[0], ce[1], ce[2], dx.data_ptr(), n, h, w, c, oh, ow, _stream()),
                  "sscg_upsample_head_bwd")
        return (dx,) + (None,) * (ctx.nin - 1)

    @staticmethod
    def _backward_b(ctx, saved, dy, g_ce, g_dice, g_bnd):
        """The backward of a node with the boundary branch: one sscg_upsample_head_bwd_b launch for whatever received a gradient (a
        boundary loss that received none leaves sdm out, and the entry runs sscg_upsample_head_bwd_h itself)."""
        x, labels, valid, coef, keys, thr, sdm, b_coef = saved
        oh, ow, weight, eps, batch = ctx.opts
        b_weight, want_ce = ctx.boundary
        use_ce = g_ce is not None and want_ce
        use_dice = g_dice is not None and coef is not None
        use_bnd = g_bnd is not None
        if dy is None and not (use_ce or use_dice or use_bnd):
            return (None,) * ctx.nin
        n, c, h, w = x.shape
        dx = empty_nhwc(n, c, h, w, x.device)
        if dy is not None:
            dy = to_nhwc(dy)
        if not use_bnd and use_ce and keys is None:
            # the unmined cross entropy is formed by the boundary instantiations only (no dl was kept): that branch rides along at zero
            g_bnd, use_bnd = torch.zeros((), dtype=torch.float32, device=x.device), True
        check(lib.sscg_upsample_head_bwd_b(x.data_ptr(), labels.data_ptr(), _ptr(keys if use_ce else None), _ptr(thr if use_ce else None),
                                           _ptr(weight), eps, _ptr(dy), _ptr(g_ce if use_ce else None), _ptr(valid if use_ce else None),
                                           _ptr(coef if use_dice else None), _ptr(g_dice if use_dice else None), batch, dx.data_ptr(),
                                           n, h, w, c, oh, ow, _ptr(sdm if use_bnd else None), _ptr(b_coef), _ptr(b_weight),
                                           _ptr(g_bnd if use_bnd else None), _stream()), "sscg_upsample_head_bwd_b")
        return (dx,) + (None,) * (ctx.nin - 1)


class UpsampleHeadFn(object):
    """The former name of the node for the head without Dice or mining, kept for code that calls its apply(): no node of its own,
    LabelHeadFn with the cross entropy wherever labels are given - (softmax map or None, loss or None)."""

    @staticmethod
    def apply(x, oh, ow, labels, want_soft, weight=None, label_smoothing=0.0):
        return LabelHeadFn.apply(x, oh, ow, labels, want_soft, labels is not None, weight, label_smoothing, None, None)[:2]


def _label_head(x, size, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, boundary=None, lovasz=None):
    """(softmax2d(interp(x)) or None, cross entropy or None, Dice loss or None[, boundary loss][, Lovasz loss]): fused (LabelHeadFn)
    when the resize grows the map, else the separate passes.  dice: a DiceOptions or None; ohem: an OhemOptions or None; boundary: a
    BoundaryLossOptions (then there is a fourth value) or None; lovasz: a LovaszOptions (then its loss is one more value, the last)
    or None."""
    oh, ow = int(size[0]), int(size[1])
    if lovasz is not None:
        if _head_applies(x, oh, ow):
            return LabelHeadFn.apply(x, oh, ow, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, boundary, lovasz)
        up = upsample_bilinear(x, size)
        out = ((softmax2d(up) if want_soft else None),
               (cross_entropy(up, labels, weight, label_smoothing, ohem=ohem) if want_ce else None),
               (dice_loss(up, labels, dice.weight, dice.smooth, dice.batch) if dice is not None else None))
        if boundary is not None:
            out = out + (boundary_loss(up, labels, boundary.weight),)
        return out + (lovasz_softmax(up, labels, lovasz),)
    if _head_applies(x, oh, ow):
        if boundary is not None:
            return LabelHeadFn.apply(x, oh, ow, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, boundary)
        return LabelHeadFn.apply(x, oh, ow, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem)
    up = upsample_bilinear(x, size)
    out = ((softmax2d(up) if want_soft else None),
           (cross_entropy(up, labels, weight, label_smoothing, ohem=ohem) if want_ce else None),
           (dice_loss(up, labels, dice.weight, dice.smooth, dice.batch) if dice is not None else None))
    return out if boundary is None else out + (boundary_loss(up, labels, boundary.weight),)


def upsample_softmax_ce(x, size, labels=None, want_soft=True, weight=None, label_smoothing=0.0, *, ohem=None):
    """(softmax2d(interp(x)) or None, CrossEntropyLoss(interp(x), labels) or None) - fused when the resize grows the map, else the
    three separate passes.  weight (functional.ce_weight's tensor) / label_smoothing: nn.CrossEntropyLoss's, on either path.
    ohem (an OhemOptions): the cross entropy runs over the mined pixels only (sscg_ohem_fwd), on either path."""
    ohem = _ohem_options(ohem) if ohem is not None and labels is not None else None
    return _label_head(x, size, labels, want_soft, labels is not None, weight, label_smoothing, None, ohem)[:2]


def upsample_softmax_ce_dice(x, size, labels, want_soft=True, weight=None, label_smoothing=0.0, dice=None, *, ohem=None):
    """upsample_softmax_ce plus the soft Dice loss of the same resized logits: (softmax2d(interp(x)) or None, cross entropy or None, Dice).
    dice: a DiceOptions (or a dict of its arguments; None = the defaults).  Fused when the resize grows the map - the head's forward
    launch, the Dice statistics and their finish; one stencil launch backward - else the separate passes.
    ohem (an OhemOptions): the cross entropy - not the Dice term - runs over the mined pixels only; still one stencil launch backward."""
    if dice is None or isinstance(dice, dict):
        dice = DiceOptions(**(dice or {}))
    if ohem is not None:
        ohem = _ohem_options(ohem)
        if not dice.ce:
            raise ValueError("ohem mines the cross entropy: DiceOptions(ce=False) leaves it nothing to mine")
    return _label_head(x, size, labels, want_soft, dice.ce, weight, label_smoothing, dice, ohem)


def upsample_softmax_losses(x, size, labels, *, want_soft=True, weight=None, label_smoothing=0.0, dice=None, ohem=None, boundary=None,
                            want_ce=True, lovasz=None):
    """The label head with every loss it knows: (softmax2d(interp(x)) or None, cross entropy or None, Dice or None, boundary loss or
    None) of the same resized logits - None for what was not asked.  weight / label_smoothing / ohem: the cross entropy's, as in
    upsample_softmax_ce; dice: a DiceOptions (or a dict of its arguments), its `ce` flag and want_ce both gate the cross entropy;
    boundary: a BoundaryLossOptions (or a dict).  Fused when the resize grows the map - still one autograd node: the existing forward
    entries, then sscg_sdm and sscg_boundary_loss_fwd; ONE sscg_upsample_head_bwd_b launch backward - else the separate passes on
    upsample_bilinear's output.  lovasz: a LovaszOptions (or a dict) - given, and only then, there is a fifth value, the
    Lovasz-softmax loss (sscg_lovasz_fwd); its gradient reaches the same backward launch as an upstream gradient of the softmax map."""
    if isinstance(dice, dict):
        dice = DiceOptions(**dice)
    want_ce = bool(want_ce) and (dice is None or dice.ce)
    if ohem is not None:
        ohem = _ohem_options(ohem)
        if not want_ce:
            raise ValueError("ohem mines the cross entropy: without it there is nothing to mine")
    if lovasz is not None:
        # one more value, the last: the Lovasz-softmax loss (its gradient rides in the same backward launch as dy_soft)
        lovasz = _lovasz_options(lovasz)
        if boundary is None:
            out = _label_head(x, size, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, None, lovasz)
            return out[:3] + (None,) + out[3:]
        return _label_head(x, size, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, _boundary_options(boundary), lovasz)
    if boundary is None:
        return _label_head(x, size, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem) + (None,)
    return _label_head(x, size, labels, want_soft, want_ce, weight, label_smoothing, dice, ohem, _boundary_options(boundary))


# ----------------------------------------------------------------------------- the unlabelled head (opt-in; include/sscg.h: sscg_unl_fwd)
class UnlabelledOptions(object):
    """The losses of the unlabelled head: the weights of the entropy, the max-squares loss and the pseudo-label cross entropy (each
    finite and >= 0; 0 = that term is not used) and the confidence threshold of the pseudo labels, in [0, 1].  The functions below
    return the three losses unweighted: the weights are the caller's (model.step adds them to its weighted sum), and `pseudo` > 0 is
    what makes the forward keep the pseudo-label map its cross entropy's backward reads."""
    __slots__ = ("entropy", "maxsq", "pseudo", "thresh")

    def __init__(self, entropy=0.0, maxsq=0.0, pseudo=0.0, thresh=0.9):
        import math
        vals = []
        for name, v in (("entropy", entropy), ("maxsq", maxsq), ("pseudo", pseudo)):
            f = float(v)
            if not (math.isfinite(f) and f >= 0.0):
                raise ValueError("unlabelled %s weight %r is not a finite number >= 0" % (name, v))
            vals.append(f)
        t = float(thresh)
        if not 0.0 <= t <= 1.0:
            raise ValueError("unlabelled pseudo-label thresh %r is outside [0, 1]" % (thresh,))
        self.entropy, self.maxsq, self.pseudo = vals
        self.thresh = t

    @property
    def any(self):
        return self.entropy > 0.0 or self.maxsq > 0.0 or self.pseudo > 0.0


def _unl_options(unl):
    if unl is None or isinstance(unl, dict):
        unl = UnlabelledOptions(**(unl or {}))
    if not isinstance(unl, UnlabelledOptions):
        raise TypeError("unl must be a functional.UnlabelledOptions (or a dict of its arguments), not %r" % (unl,))
    return unl


def unl_fwd(x, size, thresh, want_pseudo=True):
    """sscg_unl_fwd on channels-last fp32 logits x [N,C,H,W] (size = (OH, OW); (H, W): the flat form): (losses fp32 [3] = (entropy,
    max-squares, pseudo-label cross entropy), sums fp64 [4] = (sum H, sum sum p^2, sum of the kept cross entropies, K), the pseudo-label
    map uint8 [N,OH,OW] - 255 = dropped - or None).  No autograd: unlabelled_losses / upsample_softmax_unl wrap it."""
    n, c, h, w = x.shape
    oh, ow = int(size[0]), int(size[1])
    losses = torch.empty((3,), dtype=torch.float32, device=x.device)
    sums = torch.empty((4,), dtype=torch.float64, device=x.device)
    pseudo = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device) if want_pseudo else None
    ws = torch.empty(lib.sscg_unl_workspace(n, oh, ow), dtype=torch.uint8, device=x.device)
    check(lib.sscg_unl_fwd(x.data_ptr(), n, h, w, c, oh, ow, float(thresh), losses.data_ptr(), sums.data_ptr(), _ptr(pseudo),
                           ws.data_ptr(), ws.numel(), _stream()), "sscg_unl_fwd")
    return losses, sums, pseudo


def _unl_outputs(ctx, losses, sums, pseudo):
    """What both nodes return behind the softmax map: the three losses, then the sums and the map as constants.  Without the map the
    pseudo-label cross entropy is a value only: its backward has no labels to read."""
    l_ent, l_msq, l_pl = losses.unbind(0)
    ctx.mark_non_differentiable(sums, *((pseudo,) if pseudo is not None else (l_pl,)))
    # a loss nothing differentiates: backward gets None and passes NULL, that branch adds nothing
    ctx.set_materialize_grads(False)
    return l_ent, l_msq, l_pl, sums, pseudo


class UnlabelledLossFn(torch.autograd.Function):
    """The three losses of full-resolution logits [N,C,H,W] (include/sscg.h: sscg_unl_fwd / sscg_unl_bwd): (entropy, max-squares,
    pseudo-label cross entropy, sums, pseudo-label map or None)."""

    @staticmethod
    def forward(ctx, logits, thresh, keep_map):
        _need_hip(logits, f32_only=True)
        logits = to_nhwc(logits)
        losses, sums, pseudo = unl_fwd(logits, logits.shape[2:], thresh, keep_map)
        ctx.save_for_backward(logits, sums, pseudo)
        return _unl_outputs(ctx, losses, sums, pseudo)

    @staticmethod
    def backward(ctx, g_ent, g_msq, g_pl, _sums=None, _map=None):
        logits, sums, pseudo = ctx.saved_tensors
        if pseudo is None:
            g_pl = None
        if g_ent is None and g_msq is None and g_pl is None:
            return None, None, None
        n, c, h, w = logits.shape
        dx = torch.empty_like(logits, memory_format=CL)
        check(lib.sscg_unl_bwd(logits.data_ptr(), _ptr(pseudo), n, h, w, c, _ptr(g_ent), _ptr(g_msq), _ptr(g_pl), sums.data_ptr(),
                               dx.data_ptr(), _stream()), "sscg_unl_bwd")
        return dx, None, None


class UnlabelledHeadFn(torch.autograd.Function):
    """interp (bilinear, align_corners=True) -> softmax2d and the three losses of the UNLABELLED prediction, from the LOW-resolution
    logits: (softmax map or None, entropy, max-squares, pseudo-label cross entropy, sums, pseudo-label map or None); the resized logits
    never reach memory.  Forward: the label head's own launch for the softmax map (_label_head_forward without labels - the bits of
    upsample_softmax_ce's map), then sscg_unl_fwd.  Backward: ONE sscg_upsample_head_bwd_u launch for the map's upstream gradient and
    every loss that received one.  No branch of this node can coexist with a label branch of LabelHeadFn: the two are separate nodes."""

    @staticmethod
    def forward(ctx, x, oh, ow, want_soft, thresh, keep_map):
        _need_hip(x, f32_only=True)
        x = to_nhwc(x)
        y = _label_head_forward(x, oh, ow, None, True, False, None, 0.0)[0] if want_soft else None
        losses, sums, pseudo = unl_fwd(x, (oh, ow), thresh, keep_map)
        ctx.size = (oh, ow)
        ctx.save_for_backward(x, sums, pseudo)
        return (y,) + _unl_outputs(ctx, losses, sums, pseudo)

    @staticmethod
    def backward(ctx, dy, g_ent, g_msq, g_pl, _sums=None, _map=None):
        x, sums, pseudo = ctx.saved_tensors
        if pseudo is None:
            g_pl = None
        if dy is None and g_ent is None and g_msq is None and g_pl is None:
            return (None,) * 6
        oh, ow = ctx.size
        n, c, h, w = x.shape
        dx = empty_nhwc(n, c, h, w, x.device)
        if dy is not None:
            dy = to_nhwc(dy)
        check(lib.sscg_upsample_head_bwd_u(x.data_ptr(), _ptr(pseudo if g_pl is not None else None), _ptr(dy), _ptr(g_ent), _ptr(g_msq),
                                           _ptr(g_pl), sums.data_ptr(), dx.data_ptr(), n, h, w, c, oh, ow, _stream()),
              "sscg_upsample_head_bwd_u")
        return (dx,) + (None,) * 5


def unlabelled_losses(logits, unl=None, want_pseudo=False):
    """(entropy / ln C, max-squares loss, pseudo-label cross entropy, stats) of logits [N,C,H,W] - the model's own prediction, no labels:
    the mean over every pixel of the softmax entropy divided by ln C (in [0, 1]); -sum_c p_c^2 / 2 averaged the same way; and the cross
    entropy against the first maximum of p over the pixels where that maximum is at least unl.thresh (0 when none is).  Unweighted: the
    weights of `unl` (an UnlabelledOptions or a dict of its arguments) are the caller's.  stats = {"sums": fp64 [4] on the device = (sum
    of the entropies in nats, sum sum p^2, sum of the kept cross entropies, the kept pixels K), "pseudo": the uint8 label map with 255
    for a dropped pixel when want_pseudo, else None}.  The pseudo-label term is differentiable when unl.pseudo > 0 or want_pseudo."""
    unl = _unl_options(unl)
    l_ent, l_msq, l_pl, sums, pseudo = UnlabelledLossFn.apply(logits, unl.thresh, bool(want_pseudo) or unl.pseudo > 0.0)
    return l_ent, l_msq, l_pl, {"sums": sums, "pseudo": pseudo if want_pseudo else None}


def upsample_softmax_unl(x, size, unl=None, want_soft=True, want_pseudo=False):
    """(softmax2d(interp(x)) or None, entropy, max-squares, pseudo-label cross entropy, stats) of the unlabelled prediction's
    low-resolution logits: unlabelled_losses of the resized logits plus upsample_softmax_ce's softmax map (the same bits).  Fused when
    the resize grows the map - the head's forward launch, sscg_unl_fwd, ONE stencil launch backward - else the separate passes on
    upsample_bilinear's output."""
    unl = _unl_options(unl)
    oh, ow = int(size[0]), int(size[1])
    keep = bool(want_pseudo) or unl.pseudo > 0.0
    if _head_applies(x, oh, ow):
        soft, l_ent, l_msq, l_pl, sums, pseudo = UnlabelledHeadFn.apply(x, oh, ow, bool(want_soft), unl.thresh, keep)
    else:
        up = upsample_bilinear(x, size)
        soft = softmax2d(up) if want_soft else None
        l_ent, l_msq, l_pl, sums, pseudo = UnlabelledLossFn.apply(up, unl.thresh, keep)
    return soft, l_ent, l_msq, l_pl, {"sums": sums, "pseudo": pseudo if want_pseudo else None}


# ----------------------------------------------------------------------------- mean-teacher consistency (opt-in; include/sscg.h: sscg_teacher_fwd)
class TeacherOptions(object):
    """Mean-teacher consistency of the unlabelled head: the weights of the squared distance of the two probability maps (`mse`) and of
    the cross entropy against the teacher's hard labels (`ce`), each finite and >= 0 (0 = that term is not used); the confidence
    threshold of the teacher's labels in [0, 1] - it gates BOTH terms; the softmax temperature of the teacher, > 0 (below 1 sharpens);
    `flip`: the teacher sees each sample mirrored with probability 1/2 (model.step draws; the functions below take the bytes).  The
    functions return the two losses unweighted: the weights are the caller's."""
    __slots__ = ("mse", "ce", "thresh", "temp", "flip")

    def __init__(self, mse=0.0, ce=0.0, thresh=0.0, temp=1.0, flip=False):
        import math
        vals = []
        for name, v in (("mse", mse), ("ce", ce)):
            f = float(v)
            if not (math.isfinite(f) and f >= 0.0):
                raise ValueError("teacher %s weight %r is not a finite number >= 0" % (name, v))
            vals.append(f)
        t = float(thresh)
        if not 0.0 <= t <= 1.0:
            raise ValueError("teacher thresh %r is outside [0, 1]" % (thresh,))
        temp = float(temp)
        if not (math.isfinite(temp) and temp > 0.0):
            raise ValueError("teacher temp %r is not a finite number > 0" % (temp,))
        self.mse, self.ce = vals
        self.thresh, self.temp, self.flip = t, temp, bool(flip)

    @property
    def any(self):
        return self.mse > 0.0 or self.ce > 0.0

    @property
    def inv_temp(self):
        """1 / temp rounded to fp32 once: the factor the kernel multiplies the teacher's resized logits by."""
        return float(torch.tensor(1.0 / self.temp, dtype=torch.float32))


def _teacher_options(teacher):
    if isinstance(teacher, dict):
        teacher = TeacherOptions(**teacher)
    if not isinstance(teacher, TeacherOptions):
        raise TypeError("teacher must be a functional.TeacherOptions (or a dict of its arguments), not %r" % (teacher,))
    return teacher


def teacher_fwd(x, t, flip, size, inv_temp, thresh, want_pseudo=True, want_coef=True, table=None):
    """sscg_teacher_fwd on channels-last fp32 student logits x and teacher logits t [N,C,H,W] (size = (OH, OW); (H, W): the flat form);
    flip: uint8 [N] on the device or None.  table: an int32 [N, 8] mix table on the device (mix_boxes' rows, the box in OUTPUT pixels)
    or None - given, the call is sscg_teacher_fwd_mix: inside sample n's box the teacher is sample table[n][0]'s.  (losses fp32 [2] = (L_mse, L_ce), sums fp64 [4] = (sum_kept d, A, sum_kept ce, K), the
    teacher's label map uint8 [N,OH,OW] - 255 = dropped - or None, coef fp32 [N,OH,OW,C] = d L_mse / d p or None).  No autograd:
    upsample_softmax_teacher wraps it."""
    n, c, h, w = x.shape
    if tuple(t.shape) != (n, c, h, w) or t.dtype != torch.float32 or t.device != x.device:
        raise _lib.SscgError("teacher_fwd: the teacher's logits must match the student's %s fp32 on %s, got %s %s on %s"
                             % (tuple(x.shape), x.device, tuple(t.shape), t.dtype, t.device))
    if flip is not None and (flip.dtype != torch.uint8 or tuple(flip.shape) != (n,) or flip.device != x.device or not flip.is_contiguous()):
        raise _lib.SscgError("teacher_fwd: flip must be a contiguous uint8 [%d] tensor on %s" % (n, x.device))
    oh, ow = int(size[0]), int(size[1])
    losses = torch.empty((2,), dtype=torch.float32, device=x.device)
    sums = torch.empty((4,), dtype=torch.float64, device=x.device)
    pseudo = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device) if want_pseudo else None
    coef = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device) if want_coef else None
    if table is not None and (table.dtype != torch.int32 or tuple(table.shape) != (n, 8) or table.device != x.device or not table.is_contiguous()):
        raise _lib.SscgError("teacher_fwd: table must be a contiguous int32 [%d, 8] tensor on %s" % (n, x.device))
    ws = torch.empty(lib.sscg_teacher_workspace(n, oh, ow), dtype=torch.uint8, device=x.device)
    tail = (n, h, w, c, oh, ow, float(inv_temp), float(thresh), losses.data_ptr(), sums.data_ptr(), _ptr(pseudo), _ptr(coef), ws.data_ptr(),
            ws.numel(), _stream())
    if table is None:
        check(lib.sscg_teacher_fwd(x.data_ptr(), t.data_ptr(), _ptr(flip), *tail), "sscg_teacher_fwd")
    else:
        check(lib.sscg_teacher_fwd_mix(x.data_ptr(), t.data_ptr(), _ptr(flip), table.data_ptr(), *tail), "sscg_teacher_fwd_mix")
    return losses, sums, pseudo, coef


def _teacher_forward(ctx, x, t, flip, size, inv_temp, thresh, use_ce, want_coef, unl_thresh, unl_keep, mix=None):
    """What both teacher nodes run behind the softmax map: sscg_teacher_fwd, and sscg_unl_fwd when an --unl_* weight asks for its three
    losses; `mix`: teacher_fwd's table.  Saves (x, coef, the teacher's sums and map, sscg_unl_fwd's sums and map) and returns the node's outputs after the map:
    (L_mse, L_ce, L_ent, L_msq, L_pl, the teacher's sums and map, sscg_unl_fwd's sums) - None for what did not run."""
    t_losses, t_sums, t_map, coef = teacher_fwd(x, t, flip, size, inv_temp, thresh, True, want_coef, mix)
    l_mse, l_ce = t_losses.unbind(0)
    l_ent = l_msq = l_pl = u_sums = u_map = None
    if unl_thresh is not None:
        u_losses, u_sums, u_map = unl_fwd(x, size, unl_thresh, unl_keep and not use_ce)
        l_ent, l_msq, l_pl = u_losses.unbind(0)
    ctx.use_ce = use_ce
    ctx.save_for_backward(x, coef, t_sums, t_map, u_sums, u_map)
    # the constants, and the losses whose backward has nothing to read: the squared distance without its coefficient map, the teacher's
    # cross entropy unless it owns the pseudo-label slot, sscg_unl_fwd's without its own map
    dead = [v for v, live in ((l_mse, coef is not None), (l_ce, use_ce), (l_pl, u_map is not None)) if v is not None and not live]
    ctx.mark_non_differentiable(t_sums, t_map, *((u_sums,) if u_sums is not None else ()), *dead)
    ctx.set_materialize_grads(False)
    return l_mse, l_ce, l_ent, l_msq, l_pl, t_sums, t_map, u_sums


def _teacher_slot(ctx, g_ce, g_pl):
    """(pseudo, g, sums) of the ONE pseudo-label slot of the backward entries: the teacher's when its cross entropy is on, else
    sscg_unl_fwd's own; (None, None, some sums) when neither received a gradient."""
    _, _, t_sums, t_map, u_sums, u_map = ctx.saved_tensors
    if ctx.use_ce:
        return (t_map, g_ce, t_sums) if g_ce is not None else (None, None, t_sums)
    if u_map is not None and g_pl is not None:
        return u_map, g_pl, u_sums
    return None, None, t_sums


class TeacherHeadFn(torch.autograd.Function):
    """interp (bilinear, align_corners=True) -> softmax2d of the UNLABELLED prediction plus its consistency with a teacher's logits of
    the same shape, from the LOW-resolution logits of both: (softmax map or None, L_mse, L_ce, L_ent, L_msq, L_pl, the teacher's sums
    and label map, sscg_unl_fwd's sums or None).  Forward: the label head's own launch for the map (the bits of upsample_softmax_ce's),
    sscg_teacher_fwd, and sscg_unl_fwd when `unl_thresh` is given.  Backward: the squared distance's coefficient map joins the map's
    upstream gradient (one sscg_lovasz_scale_add), then ONE sscg_upsample_head_bwd_u launch whose pseudo-label slot is the teacher's
    (use_ce) or sscg_unl_fwd's own.  The teacher's logits, `flip` and `mix` (teacher_fwd's table: sscg_teacher_fwd_mix takes the forward's
    place, the backward is the same) are constants."""

    @staticmethod
    def forward(ctx, x, oh, ow, t, flip, want_soft, inv_temp, thresh, use_ce, want_coef, unl_thresh, unl_keep, mix=None):
        _need_hip(x, f32_only=True)
        x, t = to_nhwc(x), to_nhwc(t)
        y = _label_head_forward(x, oh, ow, None, True, False, None, 0.0)[0] if want_soft else None
        ctx.size = (oh, ow)
        return (y,) + _teacher_forward(ctx, x, t, flip, (oh, ow), inv_temp, thresh, use_ce, want_coef, unl_thresh, unl_keep, mix)

    @staticmethod
    def backward(ctx, dy, g_mse, g_ce, g_ent, g_msq, g_pl, *_consts):
        x, coef = ctx.saved_tensors[:2]
        pseudo, g_slot, sums = _teacher_slot(ctx, g_ce, g_pl)
        if coef is None:
            g_mse = None
        if dy is None and g_mse is None and g_ent is None and g_msq is None and g_slot is None:
            return (None,) * 13
        if dy is not None:
            dy = to_nhwc(dy)
        if g_mse is not None:
            dy = _lovasz_upstream(coef, g_mse.contiguous(), dy)
        oh, ow = ctx.size
        n, c, h, w = x.shape
        dx = empty_nhwc(n, c, h, w, x.device)
        check(lib.sscg_upsample_head_bwd_u(x.data_ptr(), _ptr(pseudo), _ptr(dy), _ptr(g_ent), _ptr(g_msq), _ptr(g_slot), sums.data_ptr(),
                                           dx.data_ptr(), n, h, w, c, oh, ow, _stream()), "sscg_upsample_head_bwd_u")
        return (dx,) + (None,) * 12


class TeacherLossFn(torch.autograd.Function):
    """The flat form, where the fused head does not apply: the same values from full-resolution logits `up` and teacher logits of the
    same size, and from `soft` = softmax2d(up) (a node of its own; None when the squared distance is off), which this node does not
    read - it is where that term's gradient goes: g_mse * coef is `soft`'s gradient (sscg_lovasz_scale_add) and SoftmaxFn's
    sscg_softmax_bwd carries it on; every other live term is one sscg_unl_bwd launch on `up`."""

    @staticmethod
    def forward(ctx, up, soft, t, flip, inv_temp, thresh, use_ce, unl_thresh, unl_keep, mix=None):
        _need_hip(up, f32_only=True)
        up, t = to_nhwc(up), to_nhwc(t)
        return _teacher_forward(ctx, up, t, flip, up.shape[2:], inv_temp, thresh, use_ce, soft is not None, unl_thresh, unl_keep, mix)

    @staticmethod
    def backward(ctx, g_mse, g_ce, g_ent, g_msq, g_pl, *_consts):
        up, coef = ctx.saved_tensors[:2]
        pseudo, g_slot, sums = _teacher_slot(ctx, g_ce, g_pl)
        d_soft = d_up = None
        if coef is not None and g_mse is not None:
            d_soft = _lovasz_upstream(coef, g_mse.contiguous(), None)
        if g_ent is not None or g_msq is not None or g_slot is not None:
            n, c, h, w = up.shape
            d_up = torch.empty_like(up, memory_format=CL)
            check(lib.sscg_unl_bwd(up.data_ptr(), _ptr(pseudo), n, h, w, c, _ptr(g_ent), _ptr(g_msq), _ptr(g_slot), sums.data_ptr(),
                                   d_up.data_ptr(), _stream()), "sscg_unl_bwd")
        return (d_up, d_soft) + (None,) * 8


def upsample_softmax_teacher(x, size, teacher_logits, teacher, unl=None, flip=None, want_soft=True, mix=None):
    """(softmax2d(interp(x)) or None, L_mse, L_ce, L_ent, L_msq, L_pl, stats): the unlabelled prediction's softmax map (the bits of
    upsample_softmax_ce's) and its consistency with `teacher_logits` - the low-resolution logits, shaped like x, of a teacher that saw
    the same batch, sample n mirrored on W where flip[n] (uint8 [N] on the device, or None) is set.  teacher: a TeacherOptions (or a
    dict); L_mse = the squared distance of the two probability maps over the pixels the teacher is confident on, divided by C V;
    L_ce = the student's cross entropy against the teacher's first maximum over the same pixels, divided by their number.  Unweighted.
    unl: an UnlabelledOptions with a weight (or None): L_ent, L_msq and L_pl are upsample_softmax_unl's, else None; both pseudo-label
    terms at once are refused - the backward has one pseudo-label slot and the teacher's labels are the better source.  stats = {"sums":
    fp64 [4] = (sum_kept d, A = agreeing kept pixels, sum_kept ce, K), "pseudo": the teacher's uint8 label map, 255 = dropped,
    "unl_sums": sscg_unl_fwd's sums or None}.  No gradient reaches the teacher.  Fused when the resize grows the map - ONE stencil
    launch backward - else the separate passes on upsample_bilinear's output.
    mix: an int32 [N, 8] table on the device (mix_boxes' rows, drawn at `size`) or None - the CutMix consistency: x is the student's
    prediction of mix_boxes(batch, table), teacher_logits the teacher's of the UNMIXED batch, and inside sample n's box the student
    is held to the teacher's prediction of sample table[n][0] (sscg_teacher_fwd_mix: the same mix of the teacher's maps, which are
    never written at the output size).  A constant, like flip."""
    teacher = _teacher_options(teacher)
    unl = _unl_options(unl) if unl is not None else None
    if unl is not None and not unl.any:
        unl = None
    use_ce = teacher.ce > 0.0
    if use_ce and unl is not None and unl.pseudo > 0.0:
        raise ValueError("teacher ce and unl pseudo are both > 0: the head's backward has one pseudo-label slot, and the teacher's labels "
                         "are the better source of the same term")
    if teacher_logits.requires_grad:
        teacher_logits = teacher_logits.detach()
    oh, ow = int(size[0]), int(size[1])
    unl_thresh = unl.thresh if unl is not None else None
    unl_keep = unl is not None and unl.pseudo > 0.0
    want_coef = teacher.mse > 0.0
    if _head_applies(x, oh, ow):
        out = TeacherHeadFn.apply(x, oh, ow, teacher_logits, flip, bool(want_soft), teacher.inv_temp, teacher.thresh, use_ce, want_coef,
                                  unl_thresh, unl_keep, mix)
    else:
        up = upsample_bilinear(x, size)
        soft = softmax2d(up) if want_soft or want_coef else None
        out = (soft if want_soft else None,) + TeacherLossFn.apply(up, soft if want_coef else None, upsample_bilinear(teacher_logits, size),
                                                                   flip, teacher.inv_temp, teacher.thresh, use_ce, unl_thresh, unl_keep, mix)
    soft, l_mse, l_ce, l_ent, l_msq, l_pl, t_sums, t_map, u_sums = out
    return soft, l_mse, l_ce, l_ent, l_msq, l_pl, {"sums": t_sums, "pseudo": t_map, "unl_sums": u_sums}


# ----------------------------------------------------------------------------- the gated CRF loss (opt-in; include/sscg.h: sscg_crf_loss_fwd)
def _crf_loss_options(crf):
    """None = CrfOptions(): the UNTUNED defaults of the inference CRF, which nobody has tuned for training either."""
    if crf is None:
        return CrfOptions()
    if isinstance(crf, dict):
        crf = CrfOptions(**crf)
    if not isinstance(crf, CrfOptions):
        raise TypeError("crf must be a functional.CrfOptions (or a dict of its arguments), not %r" % (crf,))
    return crf


def crf_loss_fwd(p, image, crf, want_coef=True):
    """sscg_crf_loss_fwd on a channels-last fp32 softmax map p [N,C,OH,OW] and a channels-last guide image [N,IC,OH,OW]: (loss, sums fp64
    [2] = (sum e, sum ksum), coef fp32 [N,OH,OW,C] = d loss / d p or None).  No autograd: crf_loss wraps it."""
    n, c, oh, ow = p.shape
    loss = _scalar(p.device)
    sums = torch.empty((2,), dtype=torch.float64, device=p.device)
    coef = torch.empty((n, oh, ow, c), dtype=torch.float32, device=p.device) if want_coef else None
    ws = torch.empty(lib.sscg_crf_loss_workspace(n, oh, ow), dtype=torch.uint8, device=p.device)
    check(lib.sscg_crf_loss_fwd(p.data_ptr(), n, oh, ow, c, image.data_ptr(), int(image.shape[1]), C.byref(crf.params()), loss.data_ptr(),
                                sums.data_ptr(), _ptr(coef), ws.data_ptr(), ws.numel(), _stream()), "sscg_crf_loss_fwd")
    return loss, sums, coef


class CrfLossFn(torch.autograd.Function):
    """The gated CRF loss of a softmax map [N,C,OH,OW] under a guide image [N,IC,OH,OW] (include/sscg.h: sscg_crf_loss_fwd).  The loss
    is quadratic in the map and the pairwise weight symmetric, so the forward leaves d loss / d p - kept only when the map needs a
    gradient - and the backward is one sscg_lovasz_scale_add launch on it.  The image gets no gradient."""

    @staticmethod
    def forward(ctx, probs, image, crf):
        _need_hip(probs, f32_only=True)
        _need_hip(image, f32_only=True)
        loss, _, coef = crf_loss_fwd(to_nhwc(probs), to_nhwc(image), crf, ctx.needs_input_grad[0])
        ctx.save_for_backward(coef)
        return loss

    @staticmethod
    def backward(ctx, g):
        (coef,) = ctx.saved_tensors
        return _lovasz_upstream(coef, g.contiguous(), None), None, None


def crf_loss(probs, image, crf=None):
    """The gated (relaxed dense) CRF loss (Tang et al., ECCV 2018; Obukhov et al., 2019) of the softmax map `probs` fp32 [N,C,OH,OW]
    guided by `image` fp32 [N,IC,OH,OW] (IC <= 4, the map's size): the mean over the pixels of sum_j k(i, j) (1 - p(i) . p(j)) over the
    dilated window of `crf` - a CrfOptions, a dict of its arguments, or None for CrfOptions(), whose defaults are UNTUNED for training
    as they are for inference; its `iterations` is not used.  Differentiable in `probs` only."""
    crf = _crf_loss_options(crf)
    _need_hip(probs, f32_only=True)
    _need_hip(image, f32_only=True)
    if probs.dim() != 4 or image.dim() != 4:
        raise _lib.SscgError("crf_loss: a 4-D softmax map and a 4-D guide image expected")
    n, c, oh, ow = probs.shape
    if tuple(image.shape) != (n, image.shape[1], oh, ow) or not 1 <= image.shape[1] <= 4:
        raise _lib.SscgError("crf_loss: the guide image must be [N, 1..4, OH, OW] at the map's size, got %s" % (tuple(image.shape),))
    return CrfLossFn.apply(probs, image.detach(), crf)


class MSEConstFn(torch.autograd.Function):
    """nn.MSELoss()(x, full_like(x, target)) - the LSGAN terms."""

    @staticmethod
    def forward(ctx, x, target):
        _need_hip(x, f32_only=True)
        if not (x.is_contiguous() or x.is_contiguous(memory_format=CL)):
            x = x.contiguous()
        loss = _scalar(x.device)
        ws = _loss_ws(x.device)
        check(lib.sscg_mse_const_fwd(x.data_ptr(), x.numel(), target, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "sscg_mse_const_fwd")
        ctx.target = target
        ctx.save_for_backward(x)
        return loss

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x, memory_format=torch.preserve_format)
        check(lib.sscg_mse_const_bwd(x.data_ptr(), x.numel(), ctx.target, g.data_ptr(), 1.0, dx.data_ptr(), _stream()),
              "sscg_mse_const_bwd")
        return dx, None


class L1Fn(torch.autograd.Function):
    """nn.L1Loss()(a, b); gradient flows to `a` only (b is data in the reference, model.py:461)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_hip(a, f32_only=True)
        _need_hip(b, f32_only=True)
        a, b = to_nhwc(a), to_nhwc(b)
        loss = _scalar(a.device)
        ws = _loss_ws(a.device)
        check(lib.sscg_l1_fwd(a.data_ptr(), b.data_ptr(), a.numel(), loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "sscg_l1_fwd")
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a, memory_format=CL)
        check(lib.sscg_l1_bwd(a.data_ptr(), b.data_ptr(), a.numel(), g.data_ptr(), 1.0, da.data_ptr(), _stream()), "sscg_l1_bwd")
        return da, None


class SsimOptions(object):
    """The structural-similarity term of l1_ssim_loss / ssim_loss / ssim (include/sscg.h: sscg_l1_ssim_fwd): a window x window
    Gaussian of `sigma` (window odd, 3..11), data_range L = max - min of the images ([-1, 1] after Normalize(.5, .5): 2), which sets
    c1 = (0.01 L)^2 and c2 = (0.03 L)^2."""
    __slots__ = ("window", "sigma", "data_range")

    def __init__(self, window=11, sigma=1.5, data_range=2.0):
        if isinstance(window, bool) or int(window) != window or not (3 <= int(window) <= 11) or int(window) % 2 == 0:
            raise ValueError("ssim window %r must be an odd integer in 3..11" % (window,))
        if not (float(sigma) > 0.0 and math.isfinite(float(sigma))):
            raise ValueError("ssim sigma %r must be a finite number > 0" % (sigma,))
        if not (float(data_range) > 0.0 and math.isfinite(float(data_range))):
            raise ValueError("ssim data_range %r must be a finite number > 0" % (data_range,))
        self.window, self.sigma, self.data_range = int(window), float(sigma), float(data_range)

    @property
    def c1(self):
        return (0.01 * self.data_range) ** 2

    @property
    def c2(self):
        return (0.03 * self.data_range) ** 2


def _ssim_options(ssim):
    if ssim is None:
        return SsimOptions()
    if isinstance(ssim, dict):
        ssim = SsimOptions(**ssim)
    if not isinstance(ssim, SsimOptions):
        raise TypeError("ssim must be a functional.SsimOptions (or a dict of its arguments), not %r" % (ssim,))
    return ssim


def _ssim_operands(a, b, opts):
    _need_hip(a, f32_only=True)
    _need_hip(b, f32_only=True)
    if a.dim() != 4 or a.shape != b.shape:
        raise _lib.SscgError("ssim: two [N, C, H, W] tensors of one shape expected, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if min(a.shape[2], a.shape[3]) < opts.window:
        raise _lib.SscgError("ssim: a %dx%d image is smaller than the %d-pixel window" % (a.shape[2], a.shape[3], opts.window))
    return to_nhwc(a), to_nhwc(b)


def l1_ssim_fwd(a, b, opts, want_l1=True, want_coef=False, want_per_sample=False):
    """sscg_l1_ssim_fwd on channels-last fp32 a, b [N,C,H,W]: (l1 or None, ssim_loss, per_sample [N] or None, coef or None), coef =
    the backward's three coefficient maps [3,N,H',W',C].  No autograd."""
    n, c, h, w = a.shape
    k = opts.window
    dev = a.device
    l1 = _scalar(dev) if want_l1 else None
    loss = _scalar(dev)
    per = torch.empty((n,), dtype=torch.float32, device=dev) if want_per_sample else None
    coef = torch.empty((3, n, h - k + 1, w - k + 1, c), dtype=torch.float32, device=dev) if want_coef else None
    ws = _WS.get(lib.sscg_ssim_workspace(n, h, w, c, k), dev)
    check(lib.sscg_l1_ssim_fwd(a.data_ptr(), b.data_ptr(), n, h, w, c, k, opts.sigma, opts.c1, opts.c2, _ptr(l1), loss.data_ptr(),
                               _ptr(per), _ptr(coef), ws.data_ptr(), ws.numel(), _stream()), "sscg_l1_ssim_fwd")
    return l1, loss, per, coef


class L1SsimFn(torch.autograd.Function):
    """nn.L1Loss()(a, b) and 1 - mean SSIM(a, b) from one forward launch; one backward launch writes the whole gradient of both to `a`
    (b is data).  want_l1 False: the SSIM term alone."""

    @staticmethod
    def forward(ctx, a, b, opts, want_l1):
        a, b = _ssim_operands(a, b, opts)
        need = ctx.needs_input_grad[0]
        l1, loss, _, coef = l1_ssim_fwd(a, b, opts, want_l1=want_l1, want_coef=need)
        ctx.opts, ctx.want_l1 = opts, want_l1
        ctx.set_materialize_grads(False)             # an output nothing reads arrives as None: its term is not formed
        if need:
            ctx.save_for_backward(a, b, coef)
        return (l1, loss) if want_l1 else loss

    @staticmethod
    def backward(ctx, *gs):
        a, b, coef = ctx.saved_tensors
        g_l1, g_ssim = gs if ctx.want_l1 else (None, gs[0])
        n, c, h, w = a.shape
        da = torch.empty_like(a, memory_format=CL)
        check(lib.sscg_l1_ssim_bwd(a.data_ptr(), b.data_ptr(), coef.data_ptr(), n, h, w, c, ctx.opts.window, ctx.opts.sigma, _ptr(g_l1), 1.0,
                                   _ptr(g_ssim), 1.0, da.data_ptr(), _stream()), "sscg_l1_ssim_bwd")
        return da, None, None, None


class MseFn(torch.autograd.Function):
    """nn.MSELoss()(a, b) between two tensors (utils.perceptual_loss, utils.py:205-206); gradients to both."""

    @staticmethod
    def forward(ctx, a, b):
        _need_hip(a, f32_only=True)
        _need_hip(b, f32_only=True)
        a, b = to_nhwc(a), to_nhwc(b)
        loss = _scalar(a.device)
        ws = _loss_ws(a.device)
        check(lib.sscg_mse_fwd(a.data_ptr(), b.data_ptr(), a.numel(), loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sscg_mse_fwd")
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a, memory_format=CL)
        db = torch.empty_like(b, memory_format=CL) if ctx.needs_input_grad[1] else None
        check(lib.sscg_mse_bwd(a.data_ptr(), b.data_ptr(), a.numel(), g.data_ptr(), 1.0, da.data_ptr(), _ptr(db), _stream()), "sscg_mse_bwd")
        return da, db


def mse_loss(a, b):
    return MseFn.apply(a, b)


WSUM_MAX_TERMS = 16        # sscg_weighted_sum's cap (include/sscg.h): the terms travel in the kernel's argument block


def weighted_sum_launches(n):
    """Forward launches of `weighted_sum` over n terms: one up to the entry's cap; beyond it every further launch takes the running
    partial sum (weight 1) and the next WSUM_MAX_TERMS - 1 terms.  Any n >= 1 is served: nothing on the host path counts terms."""
    if n < 1:
        raise ValueError("weighted_sum needs at least one term (given %d)" % n)
    return 1 if n <= WSUM_MAX_TERMS else 1 + -(-(n - WSUM_MAX_TERMS) // (WSUM_MAX_TERMS - 1))


def _weighted_sum_launch(ptrs, weights, out):
    """One sscg_weighted_sum launch over the device scalars at `ptrs`.  The entry reads them through a host table, which
    racecheck.py cannot follow from the argument list: they are announced like the buffers of a batched transpose."""
    n = len(ptrs)
    tab = (C.c_void_p * n)(*ptrs)
    ws = (C.c_float * n)(*weights)
    if _NOTE_BATCH is not None:
        _NOTE_BATCH(C.addressof(tab), [(p, None) for p in ptrs])
    check(lib.sscg_weighted_sum(tab, ws, n, out.data_ptr(), _stream()), "sscg_weighted_sum")


class WeightedSumFn(torch.autograd.Function):
    """sum_i w_i * term_i over 0-dim device scalars (gen_loss, discriminator_loss), any number of them: up to WSUM_MAX_TERMS in one
    launch; more are folded in index order (weighted_sum_launches), so the value is the left-to-right fp32 sum either way."""

    @staticmethod
    def forward(ctx, weights, *terms):
        n = len(terms)
        weighted_sum_launches(n)
        ptrs = [t.data_ptr() for t in terms]
        ws = [float(w) for w in weights]
        if len(ws) != n:
            raise ValueError("weighted_sum: %d terms but %d weights" % (n, len(ws)))
        out = _scalar(terms[0].device)
        _weighted_sum_launch(ptrs[:WSUM_MAX_TERMS], ws[:WSUM_MAX_TERMS], out)
        for i in range(WSUM_MAX_TERMS, n, WSUM_MAX_TERMS - 1):
            part, out = out, _scalar(terms[0].device)
            j = i + WSUM_MAX_TERMS - 1
            _weighted_sum_launch([part.data_ptr()] + ptrs[i:j], [1.0] + ws[i:j], out)
        ctx.weights = ws
        return out

    @staticmethod
    def backward(ctx, g):
        grads = []
        for w in ctx.weights:
            gi = _scalar(g.device)
            _weighted_sum_launch([g.data_ptr()], [w], gi)
            grads.append(gi)
        return (None, *grads)


# functional spellings
def conv2d(x, w, bias=None, stride=1, pad=0, dil=1, pad_mode=PAD_ZEROS, act=ACT_NONE, slope=0.0, out_f32=True):
    """out_f32 matters in bf16 mode only: True keeps the result fp32 (network heads), False makes it a bf16 activation."""
    return Conv2dFn.apply(x, w, bias, stride, pad, dil, pad_mode, act, slope, out_f32, None, torch.is_grad_enabled())


# Eval-mode BatchNorm folded into the conv that feeds it (sscg_conv2d_fwd_affine): under .eval() the normalisation is a per-channel affine
# known before the conv starts, so a conv -> BatchNorm [+ residual] -> activation unit of an inference forward is ONE launch instead of
# three (conv, sscg_rstd_from_var, sscg_norm_apply) and its map never makes the round trip through memory.  SSCG_FUSE_EVAL_NORM=0 keeps
# the separate passes (an A/B aid: the bits are the same).
FUSE_EVAL_NORM = [os.environ.get("SSCG_FUSE_EVAL_NORM", "1") != "0"]


def _bn_eval_plan(x, w, stride, pad, dil, pad_mode, act, slope, out_f32):
    """(descriptor, weight operand) of the fused launch, or (None, None) where the library does not serve the geometry: the exact-fp32
    kernel (3-channel stems), the thin 1x1 kernels, the heads' 32-column tile classes, padded stems, tanh."""
    if act == ACT_TANH or (x.dtype == torch.float32 and _padded_stem(x.shape, w.shape, stride, pad, dil, pad_mode, 0)):
        return None, None
    if x.dtype == torch.bfloat16 and x.shape[1] % 64:
        return None, None
    wop, wdt, wplane = _fwd_operands(x, w, (stride, pad, dil, pad_mode))       # the copies conv2d uses, obtained the same way
    d = make_desc(x.shape, w.shape, stride, pad, dil, pad_mode, act, slope, _dt(x), wdt, _DT[_out_dtype(out_f32)], _prec(), wplane)
    key = (id(d), "affine")
    ok = _PLAN_SIZES.get(key)
    if ok is None:
        ok = _PLAN_SIZES[key] = bool(lib.sscg_conv2d_fwd_affine_applies(C.byref(d)))
    return (d, wop) if ok else (None, None)


def conv_bn_eval_applies(x, w, stride=1, pad=0, dil=1, pad_mode=PAD_ZEROS, act=ACT_NONE, slope=0.0, out_f32=False):
    """Does one launch serve this conv -> eval-mode BatchNorm -> activation unit (sscg_conv2d_fwd_affine_applies)?"""
    return _bn_eval_plan(x, w, stride, pad, dil, pad_mode, act, slope, out_f32)[0] is not None


def conv_bn_eval_act(x, w, bias, running_mean, running_var, gamma=None, beta=None, residual=None, stride=1, pad=0, dil=1,
                     pad_mode=PAD_ZEROS, eps=1e-5, act=ACT_NONE, slope=0.0, out_f32=False):
    """act(batch_norm(conv2d(x, w) + bias; running statistics) [+ residual]) of an inference forward (arch/generators.py:345-365 under
    model.py:555-574, validation.py, testing.py): bit for bit `batch_norm_act(conv2d(x, w, bias, ...), gamma, beta, running_mean,
    running_var, training=False, ...)`, in one launch where the library serves the geometry - and by exactly those separate passes where
    it does not.  A plain function, not an autograd node."""
    _need_hip(x)
    _no_grad_input(x, "conv_bn_eval_act")
    if residual is not None:
        _no_grad_input(residual, "conv_bn_eval_act")
    if (gamma is None) != (beta is None):
        raise _lib.SscgError("conv_bn_eval_act: gamma and beta come together")
    x = to_nhwc(x.detach())
    res = to_nhwc(residual.detach()) if residual is not None else None
    d, wop = _bn_eval_plan(x, w, stride, pad, dil, pad_mode, act, slope, out_f32)
    if d is not None and res is not None and res.dtype != _out_dtype(out_f32):
        d = None
    if d is None:
        with torch.no_grad():
            y = conv2d(x, w, bias, stride, pad, dil, pad_mode, ACT_NONE, 0.0, out_f32)
            return batch_norm_act(y, gamma, beta, running_mean, running_var, False, 0.1, eps, act, slope, res)
    y = empty_nhwc(d.N, d.K, d.P, d.Q, x.device, _out_dtype(out_f32))
    if res is not None and tuple(res.shape) != tuple(y.shape):
        raise _lib.SscgError("conv_bn_eval_act: residual %s does not match the output %s" % (tuple(res.shape), tuple(y.shape)))
    ws = _WS.get(_ws_bytes(d, "fwd"), x.device)
    _timed("fwd", d, lambda: check(lib.sscg_conv2d_fwd_affine(C.byref(d), x.data_ptr(), wop.data_ptr(), _ptr(bias), running_mean.data_ptr(),
                                                              running_var.data_ptr(), eps, _ptr(gamma), _ptr(beta), _ptr(res), y.data_ptr(),
                                                              ws.data_ptr(), ws.numel(), _stream()), "sscg_conv2d_fwd_affine"))
    return y


def backward(loss):
    """loss.backward() with the autograd engine on the CALLING thread.  Every node of these graphs launches kernels and returns
    (nothing to run in parallel on the host), while the hop to the engine's device thread costs ~10 % of a step's issue time
    (79 -> 71 ms at 64x64, batch 2).  Backward nodes still run on the stream of their forward (the engine's stream guards do
    not depend on the thread)."""
    with torch.autograd.set_multithreading_enabled(False):
        loss.backward()
    # weight / bias / norm gradients are queued per side lane in batches (run_on_side_stream(defer=True)): launch what is still
    # pending, so that a stream synchronisation after this call covers every gradient kernel of the pass (the arenas are complete
    # once the side lanes are joined: SideStream.join / FusedAdam.step)
    flush_side_work()


def conv_norm_act(x, w, bias, stride, pad, dil, pad_mode, gamma, beta, residual, running_mean, running_var, per_sample, eps, momentum,
                  act=ACT_NONE, slope=0.0):
    """conv -> norm (batch statistics) [+ residual] -> activation as one autograd node (training-mode normalisation only)."""
    return ConvNormActFn.apply(x, w, bias, gamma, beta, residual, running_mean, running_var,
                               (stride, pad, dil, pad_mode, per_sample, eps, momentum, act, slope, torch.is_grad_enabled()))


def conv2d_norm_stats(x, w, bias, stride, pad, dil, pad_mode, norm):
    """Convolution whose epilogue also produces the statistics of the normalisation layer `norm` = (per_sample, eps,
    running_mean, running_var, momentum) that follows it.  Returns (y, mean, rstd); mean/rstd None = not fused."""
    return Conv2dFn.apply(x, w, bias, stride, pad, dil, pad_mode, ACT_NONE, 0.0, False, norm, torch.is_grad_enabled())


def conv_transpose2d(x, w, bias=None, stride=1, pad=0, out_pad=0, act=ACT_NONE, slope=0.0, out_f32=False):
    return ConvTranspose2dFn.apply(x, w, bias, stride, pad, out_pad, act, slope, out_f32)


class CatChannelsFn(torch.autograd.Function):
    """torch.cat([a, b], 1) of two channels-last tensors - the skip connection of UnetSkipConnectionBlock.forward
    (arch/generators.py:44).  Device copies only (no arithmetic); the gradient is the two channel slices."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = to_nhwc(a), to_nhwc(b)
        if a.dtype != b.dtype or a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
            raise _lib.SscgError("cat_channels: tensors of one dtype, batch and spatial size expected")
        n, ca, h, w = a.shape
        ctx.ca = ca
        y = empty_nhwc(n, ca + b.shape[1], h, w, a.device, a.dtype)
        y[:, :ca].copy_(a)
        y[:, ca:].copy_(b)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = to_nhwc(dy)
        return dy[:, :ctx.ca].contiguous(memory_format=CL), dy[:, ctx.ca:].contiguous(memory_format=CL)


def cat_channels(a, b):
    return CatChannelsFn.apply(a, b)


def instance_norm_act(x, act=ACT_NONE, slope=0.0, residual=None, eps=1e-5, stats=None):
    m, r = stats if stats is not None else (None, None)
    return NormActFn.apply(x, None, None, residual, None, None, True, True, 0.0, eps, act, slope, m, r)


def batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, act=ACT_NONE, slope=0.0,
                   residual=None, groups=1, stats=None):
    """groups > 1: x holds `groups` batches stacked along N; each is normalised with its own statistics and the running
    statistics advance once per group, in order - what `groups` successive calls would compute, in one launch.
    stats = (mean, rstd) already produced by the preceding conv's epilogue (training mode)."""
    per = False if groups == 1 else int(groups)
    m, r = stats if stats is not None else (None, None)
    return NormActFn.apply(x, gamma, beta, residual, running_mean, running_var, per, training, momentum, eps, act, slope, m, r)


def upsample_bilinear(x, size):
    """nn.Upsample(size, mode='bilinear', align_corners=True) (model.py:390-392, 413-415).  A resize to the size the map already has
    (the ResnetGenerator outputs: model.py:390, :413) is the identity under align_corners=True - scale 1, every weight 1 or 0 - and so is
    its adjoint: no pass at all (it was a copy forward and a 3x3-candidate gather backward, 128 us each at 8 x 3 x 256 x 256)."""
    if x.dim() == 4 and x.shape[2] == int(size[0]) and x.shape[3] == int(size[1]):
        return x
    return UpsampleFn.apply(x, int(size[0]), int(size[1]))


def softmax2d(x):
    return SoftmaxFn.apply(x)


def cross_entropy(logits, labels, weight=None, label_smoothing=0.0, *, ohem=None):
    if ohem is not None:        # hard-pixel mining (OhemOptions): the loss over the mined pixels only
        return OhemCrossEntropyFn.apply(logits, labels, weight, label_smoothing, _ohem_options(ohem))
    return CrossEntropyFn.apply(logits, labels, weight, label_smoothing)


def mse_const(x, target):
    return MSEConstFn.apply(x, float(target))


def l1_loss(a, b):
    return L1Fn.apply(a, b)


def l1_ssim_loss(a, b, ssim=None):
    """(nn.L1Loss()(a, b), 1 - mean SSIM(a, b)) as one autograd node: one forward launch reads a and b once for both, one backward
    launch writes the gradient of both to `a`.  ssim: a SsimOptions (None = the defaults)."""
    return L1SsimFn.apply(a, b, _ssim_options(ssim), True)


def ssim_loss(a, b, ssim=None):
    """1 - mean SSIM(a, b): l1_ssim_loss without the L1 output."""
    return L1SsimFn.apply(a, b, _ssim_options(ssim), False)


def ssim(a, b, ssim=None):
    """The mean SSIM of each sample, [N] fp32.  No gradient."""
    opts = _ssim_options(ssim)
    with torch.no_grad():
        a, b = _ssim_operands(a.detach(), b.detach(), opts)
        return l1_ssim_fwd(a, b, opts, want_l1=False, want_per_sample=True)[2]


def weighted_sum(terms, weights):
    return WeightedSumFn.apply(list(weights), *terms)


if os.environ.get("SSCG_RACECHECK"):     # debug: model the autograd engine's stream hand-over for the ordering checker
    import sys as _sys
    from ._lib import dev_tool as _dev_tool
    _dev_tool("racecheck").wrap_functions(_sys.modules[__name__])
