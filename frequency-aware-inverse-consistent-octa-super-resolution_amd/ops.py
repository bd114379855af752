"""Autograd operators over the HIP kernels (include/faoctasr.h).

Each ``torch.autograd.Function`` here stands in for one ATen op class the reference's train
step executes; PyTorch supplies device memory, streams and the autograd tape,
every arithmetic kernel is ours.  Weight / affine gradients are accumulated by the kernels
straight into ``param.grad`` when that already exists (the flat gradient arena of
train.TrainStep), so no per-parameter add kernels run and the all-reduce sees one buffer.
"""
import contextlib
import ctypes
import math

import torch
from torch.autograd import Function

from . import _lib
from ._lib import call, ptr, stream_ptr

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
_ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "tanh": 3}

#: accumulate weight gradients in place into existing ``param.grad`` buffers
direct_grad = True
#: residual blocks hand the skip connection's gradient to their first convolution's input-gradient call (model._ResBlock,
#: faoctasr_conv_set_residual) instead of leaving the add to autograd; False: plain autograd (tests compare the two)
fuse_residual_grad = True


def act_code(a):
    return a if isinstance(a, int) else _ACT[a]


def _act_args(act, slope):
    """(activation code, slope) for the kernels.  Their backward takes the LeakyReLU derivative from the sign of the activation's
    OUTPUT (csrc/common.h act_grad_from_out), which is the sign of its input only while slope >= 0: a negative slope would give a
    correct forward value and a wrong gradient, so it is refused."""
    code, slope = act_code(act), float(slope)
    if code == ACT_LRELU and not slope >= 0.0:
        raise _lib.KernelError("LeakyReLU slope must be >= 0, got %r: the backward kernels read the derivative off the output's sign" % slope)
    return code, slope


def _same_shape(what, a, b):
    if a.shape != b.shape:
        raise _lib.KernelError("%s operands differ in shape: %s vs %s" % (what, tuple(a.shape), tuple(b.shape)))


def _c(t):
    if not t.is_cuda:
        raise _lib.KernelError("operand lives on %s: the HIP operators have no CPU/eager fallback" % t.device)
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------
# packed-weight images for the LDS-patch convolution kernel (include/faoctasr.h, faoctasr_conv_wpack_floats)
# ----------------------------------------------------------------------------------------
import weakref

#: bumped whenever weights change behind autograd's back and nobody knows which (``invalidate_weight_cache``); a ``ParamArena``
#: bumps only its own parameters' epoch cell (``p._fa_epoch``), so a generator update leaves the discriminators' images valid
weight_epoch = 0
use_wpack = True
#: convolution arithmetic: 0 = fp32 MFMA with Winograd F(2x2,3x3) on the stride-1 3x3 layers (default), 1 = fp32 MFMA direct only,
#: 2 = bf16x3 split operands (fp32-parity, ~5x MFMA rate); 3 = f16x2 split operands with per-tensor power-of-two scales (error at
#: or below the exact-f32 kernels', same rate as bf16x3: csrc/split16.h)
conv_precision = 0
PRECISIONS = {"f32": 0, "f32_direct": 1, "bf16x3": 2, "f16x2": 3}
#: FAOCTASR_CONV_NO_SPLIT_K (include/faoctasr.h) on every FORWARD convolution: no fp32 atomics in the forward pass, so its
#: activations -- and with them every ReLU / LeakyReLU mask the backward uses -- are bit-reproducible from run to run
reproducible_forward = False
NO_SPLIT_K = 0x100
_wpack_cache = {}
#: calls that had to pack inside the convolution call itself (state 1); a ``PackPlan`` owner watches it to learn about new images
pack_misses = 0


def invalidate_weight_cache():
    global weight_epoch
    weight_epoch += 1


# ----------------------------------------------------------------------------------------
# absmax slots of the f16x2 contraction (include/faoctasr.h: faoctasr_absmax_bits, faoctasr_conv_set_scales)
# ----------------------------------------------------------------------------------------
#: per HIP stream: (zeroed fp32 arena, cursor).  A slot is SLOT_WORDS words whose maximum is max|x| of an activation tensor (the fp32
#: bit pattern IS the float).  One arena per stream, because a slot is zeroed, filled and first read in stream order -- handing slots of one
#: arena to several streams would let a reader overtake the fill.
_scale_arenas = {}
SCALE_ARENA_SLOTS = 1024
SLOT_WORDS = 128                                # include/faoctasr.h FAOCTASR_ABSMAX_SLOT_WORDS: 8 used words, one per 64-byte line


def reset_scale_arenas():
    """Drop the arenas (their slots stay alive while something references them): the next slot comes from a freshly zeroed
    arena.  ``GraphedTrainStep`` calls it around a capture so that every slot of the graph is zeroed INSIDE the graph."""
    _scale_arenas.clear()


absmax_log = None


def _new_slot(device):
    sid = stream_ptr()
    ent = _scale_arenas.get(sid)
    if ent is None or ent[1] >= SCALE_ARENA_SLOTS or ent[0].device != device:
        ent = _scale_arenas[sid] = [torch.zeros(SCALE_ARENA_SLOTS * SLOT_WORDS, dtype=torch.float32, device=device), 0]
    i = ent[1]
    ent[1] = i + 1
    return ent[0][i * SLOT_WORDS:(i + 1) * SLOT_WORDS]


def absmax_slot(t):
    """The absmax slot of activation tensor ``t`` for a convolution enqueued on the CURRENT stream.  Cached on the tensor object for
    further uses on the same stream while the tensor is unchanged (the skip connection and the first convolution of a residual
    block read the same tensor); a producer that computes the maximum in its own epilogue may pre-set ``t._fa_absmax``."""
    sid = stream_ptr()
    c = getattr(t, "_fa_absmax", None)
    if c is not None and c[1] == t._version and c[2] == sid:
        return c[0]
    slot = _new_slot(t.device)
    call("absmax_bits", ptr(t), t.numel(), ptr(slot), sid)
    t._fa_absmax = (slot, t._version, sid)
    if absmax_log is not None:                      # (diagnostics) which tensors still need a stand-alone pass, and why
        why = "no tag" if c is None else ("version" if c[1] != t._version else "stream")
        key = (tuple(t.shape), why)
        absmax_log[key] = absmax_log.get(key, 0) + 1
    return slot


def _producer_slot(x, C, H, W):
    """A fresh absmax slot for a producer call (BatchNorm forward / backward, cat2_act forward) whose output can feed a
    split-precision convolution (>= 16 channels -- wide maps on the split kernel, narrow ones on the narrow-map kernel --, H*W a
    multiple of 4); None otherwise.  ``_producer_call`` hands it over."""
    if conv_precision != 3 or C < 16 or (H * W) & 3:
        return None
    return _new_slot(x.device)


def _producer_call(name, args, slot):
    """A producer call with ``faoctasr_out_absmax(slot)`` set immediately before it (``args`` are already evaluated: nothing that can
    raise sits between the setter and its consumer)."""
    if slot is not None:
        call("out_absmax", ptr(slot))
    call(name, *args)


def _tag_absmax(t, slot):
    """``t``'s producer has folded max|t| into ``slot`` on the current stream: ``absmax_slot(t)`` will find it."""
    if slot is not None:
        t._fa_absmax = (slot, t._version, stream_ptr())


_wgrad_ws_need = {}


def _wgrad_workspace(device, C, M, KH, KW, stride, prec):
    """Hand the CURRENT stream's scratch buffer to the next weight-gradient call (two-pass reduction of the split kernels:
    ``faoctasr_conv_set_workspace``).  Calls on one stream share the buffer; it is only live between the call's two launches."""
    if prec < 2:
        return
    key = (C, M, KH, KW, stride)
    n = _wgrad_ws_need.get(key)
    if n is None:
        n = _wgrad_ws_need[key] = _lib.load().faoctasr_conv_wgrad_workspace_floats(C, M, KH, KW, stride)
    if n > 0:
        ws = _lib.workspace(device, n + (1 << 16), tag="wgrad")
        call("conv_set_workspace", ptr(ws), ws.numel())


_gather_ws_need = {}


def _gather_workspace(device, kind, dims, reflect=0, out_pad=0):
    """Hand the CURRENT stream's scratch buffer to the next gather call (kind 0..3 as ``_needs_scales``) when its precision-3 route
    splits the reduction through one (the f16x2 narrow-map kernel: ``faoctasr_conv_gather_workspace_floats``).  Shared with the
    weight-gradient calls of the stream; it is only live between the call's two launches."""
    if conv_precision != 3:
        return
    key = (kind, dims, reflect, out_pad)
    n = _gather_ws_need.get(key)
    if n is None:
        n = _lib.load().faoctasr_conv_gather_workspace_floats(kind, *dims, reflect, out_pad)
        if n < 0:
            raise _lib.KernelError("conv_gather_workspace_floats: " + _lib.load().faoctasr_last_error().decode())
        _gather_ws_need[key] = n
    if n > 0:
        ws = _lib.workspace(device, n + (1 << 16), tag="wgrad")
        call("conv_set_workspace", ptr(ws), ws.numel())


def _conv_call(name, args, slot_a=None, slot_b=None, residual=None):
    """One convolution-type C call with its hand-over state (``faoctasr_conv_set_scales`` / ``faoctasr_conv_set_residual``: thread-local,
    consumed by the next call) set IMMEDIATELY before it: nothing that can raise -- an allocation, a pack, a pointer check -- sits
    between a setter and the call that consumes it, so a failed step cannot leave a slot or a residual pointer behind for an unrelated
    later call."""
    pa, pb, pr = ptr(slot_a), ptr(slot_b), ptr(residual)
    if pa is not None:
        call("conv_set_scales", pa, pb)
    if pr is not None:
        call("conv_set_residual", pr)
    call(name, *args)


_scale_need = {}


def _needs_scales(kind, dims, reflect=0, out_pad=0):
    """Which absmax slots the precision-3 form of a convolution-type call reads (``faoctasr_conv_needs_scales``: answered by the
    dispatch code itself): 0 = none (an exact-f32 route), 1 = slot a, 3 = both.  Cached per call signature."""
    if conv_precision != 3:
        return 0
    key = (kind, dims, reflect, out_pad)
    n = _scale_need.get(key)
    if n is None:
        n = _lib.load().faoctasr_conv_needs_scales(kind, *dims, reflect, out_pad)
        if n < 0:
            raise _lib.KernelError("conv_needs_scales: " + _lib.load().faoctasr_last_error().decode())
        _scale_need[key] = n
    return n


class _PackEntry:
    """One packed-weight image: the buffer, the gather call it belongs to (exactly the C call's arguments) and the weight
    version it holds."""
    __slots__ = ("wref", "buf", "ver", "kind", "dims", "reflect", "out_pad", "precision", "touched", "event", "ev_stream")


def _ver(w):
    cell = getattr(w, "_fa_epoch", None)
    return (w._version, weight_epoch, 0 if cell is None else cell[0], w.data_ptr(), tuple(w.shape))


def _wpack(w, kind, dims, reflect=0, out_pad=0):
    """(buffer, state, entry) for the C ABI: state 1 = pack now, 2 = buffer already holds these weights.  ``dims`` =
    (N, C, IH, IW, M, KH, KW, stride, pad) exactly as the gather call ``kind`` receives them.

    An image packed inside a convolution call (state 1) is ordered on that call's stream only.  The caller reports the launch with
    ``_packed(entry, state)``, which records an event there; a later state-2 user on ANOTHER stream waits for that event here, so the
    multi-stream schedule of ``TrainStep`` is safe on steps whose images are not covered by a ``PackPlan`` (first step, new batch
    shape: the trailing partial batch of an epoch)."""
    global pack_misses
    if not use_wpack:
        return None, 0, None
    key = (id(w), kind, conv_precision, dims, reflect, out_pad)
    ent = _wpack_cache.get(key)
    if ent is None or ent.wref() is not w:
        if len(_wpack_cache) > 4096:
            for k in [k for k, v in _wpack_cache.items() if v.wref() is None]:
                del _wpack_cache[k]
        N, C, IH, IW, M, KH, KW, stride, pad = dims
        n = _lib.load().faoctasr_conv_wpack_floats(kind, C, M, KH, KW, stride, pad, conv_precision)
        if n <= 0:
            return None, 0, None
        ent = _PackEntry()
        ent.wref, ent.buf, ent.ver = weakref.ref(w), torch.empty(n, dtype=torch.float32, device=w.device), None
        ent.event = ent.ev_stream = None
        ent.kind, ent.dims, ent.reflect, ent.out_pad, ent.precision = kind, dims, int(bool(reflect)), out_pad, conv_precision
        _wpack_cache[key] = ent
    ver = _ver(w)
    ent.touched = True
    if ent.ver == ver:
        if ent.event is not None:
            cur = torch.cuda.current_stream()
            if cur.cuda_stream != ent.ev_stream:         # packed inline on another stream: order this reader behind that launch
                if wait_guard is not None:
                    wait_guard(cur.cuda_stream, ent.ev_stream)
                cur.wait_event(ent.event)
        return ent.buf, 2, ent
    ent.ver = ver
    pack_misses += 1
    return ent.buf, 1, ent


def _packed(ent, state):
    """After a convolution call that received ``state`` 1: remember where (stream) and when (event) the image was written."""
    if state == 1:
        cur = torch.cuda.current_stream()
        ent.event, ent.ev_stream = cur.record_event(), cur.cuda_stream


def clear_touched():
    """Forget which images earlier steps used: the next ``PackPlan`` then holds exactly the images of the step run in between."""
    for e in _wpack_cache.values():
        e.touched = False


class PackPlan:
    """Every packed-weight image of a set of parameters in one launch (``faoctasr_conv_pack_job`` / ``faoctasr_conv_pack_run``,
    csrc/conv_pack.hip): the images the last step used (``touched``) at ``precision``, for weights in ``params``.  ``run()``
    packs them all and marks them current, so the convolution calls that follow pass ``wpack_state`` 2."""

    def __init__(self, params, precision):
        lib = _lib.load()
        ids = {id(p) for p in params}
        slot = ctypes.create_string_buffer(_lib.PACK_JOB_BYTES)
        blobs, base, self.entries, device = [], 0, [], None
        self.precision = precision
        for key, e in list(_wpack_cache.items()):
            w = e.wref()
            if w is None or id(w) not in ids or e.precision != precision or not e.touched:
                continue
            e.touched = False
            n = lib.faoctasr_conv_pack_job(slot, base, e.kind, w.data_ptr(), e.buf.data_ptr(), *e.dims, e.reflect, e.out_pad, e.precision)
            if n < 0:
                raise _lib.KernelError("conv_pack_job: " + lib.faoctasr_last_error().decode())
            self.entries.append((e, w.data_ptr()))     # n == 0: the call never reads its image (64->1 head): nothing to pack, still "current"
            if n > 0:
                blobs.append(slot.raw)
                base += n
                device = w.device
        self.njobs, self.nblocks = len(blobs), base
        self.table = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.float32).to(device) if blobs else None   # raw bytes, carried as fp32

    def run(self, aside=None):
        """False (nothing launched) when a weight has moved or died since the jobs were recorded: the owner drops the plan.

        ``aside``: a stream to pack on instead of the current one (ordered behind the current stream's work so far).  Readers on that
        stream see the images in stream order; readers on any other stream are ordered behind the launch by the event ``_wpack``
        already honours for images packed inside a convolution call."""
        live = [(e, e.wref()) for e, _ in self.entries]
        if any(w is None or w.data_ptr() != p for (e, w), (_, p) in zip(live, self.entries)):
            return False
        event = ev_stream = None
        if self.njobs:
            if aside is not None:
                cur = torch.cuda.current_stream()
                if cur.cuda_stream == aside.cuda_stream:
                    aside = None
                else:
                    aside.wait_stream(cur)
            with torch.cuda.stream(aside) if aside is not None else contextlib.nullcontext():
                if self.precision == 3:             # f16x2 images: the weights' absmax slots first
                    call("conv_pack_scales", ptr(self.table), self.njobs, stream_ptr())
                call("conv_pack_run", ptr(self.table), self.njobs, self.nblocks, stream_ptr())
                if aside is not None:
                    event, ev_stream = aside.record_event(), aside.cuda_stream
        for e, w in live:
            e.ver = _ver(w)
            e.event, e.ev_stream = event, ev_stream      # None: written on the stream every role of the step forks from
        return True


#: Set by TrainStep for the span of a backward pass: weight / bias gradients that accumulate straight into the gradient arena are
#: then enqueued on this second HIP stream (ordered after the producing stream's work so far), so that they overlap the
#: input-gradient chain, the BatchNorm backward passes and each other's launch tails instead of queueing behind them.
#: ``join_wgrad_stream`` makes the current stream wait for them (before the all-reduce / optimizer step).  Their operands stay
#: referenced until then, so the caching allocator cannot hand an activation to another kernel while a side-stream kernel still
#: reads it.
wgrad_stream = None
_wgrad_keep = {}
#: ``f(waiter_stream_id, waited_stream_id)`` called before each cross-stream wait issued here (train._CaptureGuard.edge)
wait_guard = None


#: (captured steps, TrainStep.capture_side_wgrad == "deferred") collect the weight-gradient launches of a backward pass and enqueue
#: them on the side stream in ONE batch when the pass is over (``end_wgrad``): one fork and one join per backward pass in the graph
#: instead of one per weight gradient
wgrad_defer = False
_deferred = []


def end_wgrad():
    """Close a ``wgrad_stream`` scope: enqueue what ``wgrad_defer`` held back, then reset the stream."""
    global wgrad_stream
    side, held = wgrad_stream, list(_deferred)
    del _deferred[:]
    wgrad_stream = None
    if held and side is not None:
        seen = {side.cuda_stream}
        for _, _, src in held + [(None, None, torch.cuda.current_stream())]:      # every stream a held launch's operands came from
            if src.cuda_stream not in seen:
                seen.add(src.cuda_stream)
                if wait_guard is not None:
                    wait_guard(side.cuda_stream, src.cuda_stream)
                side.wait_stream(src)
        with torch.cuda.stream(side):
            for fn, operands, _ in held:
                fn(side.cuda_stream)
                _wgrad_keep.setdefault(side.cuda_stream, []).append(operands)
    elif held:
        for fn, _, _ in held:
            fn(stream_ptr())


def _enqueue_wgrad(fn, *operands):
    """``fn(stream_pointer)`` on ``wgrad_stream`` when one is set, otherwise on the current stream."""
    side = wgrad_stream
    if side is None:
        fn(stream_ptr())
        return
    if wgrad_defer:
        _deferred.append((fn, operands, torch.cuda.current_stream()))
        return
    cur = torch.cuda.current_stream()
    if cur.cuda_stream != side.cuda_stream:
        if wait_guard is not None:
            wait_guard(side.cuda_stream, cur.cuda_stream)
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn(side.cuda_stream)
    _wgrad_keep.setdefault(side.cuda_stream, []).append(operands)


def join_wgrad_stream(side):
    """The current stream waits for everything enqueued on ``side``; the operands held for it are released."""
    if side is not None:
        cur = torch.cuda.current_stream()
        if cur.cuda_stream != side.cuda_stream:
            if wait_guard is not None:
                wait_guard(cur.cuda_stream, side.cuda_stream)
            cur.wait_stream(side)
        _wgrad_keep.pop(side.cuda_stream, None)


def _grad_target(p):
    g = p.grad
    if direct_grad and g is not None and g.is_contiguous() and g.dtype == torch.float32:
        return g
    return None


# ----------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------
class _Conv2d(Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, reflect, act, slope, link=None):
        """``link``: the dict a residual block shares between its first convolution and its last BatchNorm (``model._ResBlock``): the
        BatchNorm's backward leaves the skip connection's gradient there (``link["dres"]``) instead of returning it to autograd, and
        this convolution's input gradient is computed as dgrad(dy) + dres in one kernel (``faoctasr_conv_set_residual``)."""
        ctx.link = link
        x, w = _c(x), _c(w)
        N, C, IH, IW = x.shape
        M, Cw, KH, KW = w.shape
        if Cw != C:
            raise _lib.KernelError("conv2d: input has %d channels, weight expects %d" % (C, Cw))
        OH, OW = (IH + 2 * pad - KH) // stride + 1, (IW + 2 * pad - KW) // stride + 1
        if OH <= 0 or OW <= 0:
            raise RuntimeError("Calculated padded input size per channel: (%d x %d). Kernel size: (%d x %d). "
                               "Kernel size can't be greater than actual input size" % (IH + 2 * pad, IW + 2 * pad, KH, KW))
        y = torch.empty((N, M, OH, OW), dtype=torch.float32, device=x.device)
        wp, wst, ent = _wpack(w, 0, (N, C, IH, IW, M, KH, KW, stride, pad), reflect)
        sx = absmax_slot(x) if _needs_scales(0, (N, C, IH, IW, M, KH, KW, stride, pad), reflect) else None
        _gather_workspace(x.device, 0, (N, C, IH, IW, M, KH, KW, stride, pad), reflect)
        _conv_call("conv2d_fwd", (ptr(x), ptr(w), ptr(bias), ptr(y), N, C, IH, IW, M, KH, KW, stride, pad, reflect, act, slope, ptr(wp), wst,
                                  conv_precision | (NO_SPLIT_K if reproducible_forward else 0), stream_ptr()), sx)
        _packed(ent, wst)
        ctx.sx = sx
        ctx.save_for_backward(x, w, y if act else None)
        ctx.w_ref, ctx.b_ref = w, bias
        ctx.cfg = (stride, pad, reflect, act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, reflect, act, slope = ctx.cfg
        dy = _c(dy)
        st = stream_ptr()
        N, C, IH, IW = x.shape
        M, _, KH, KW = w.shape
        if act:
            g = torch.empty_like(dy)
            call("act_bwd", ptr(dy), ptr(y), ptr(g), dy.numel(), act, slope, st)
            dy = g
        dx = dw = db = None
        dg_dims = (N, C, IH + 2 * pad, IW + 2 * pad, M, KH, KW, stride, 0) if reflect else (N, C, IH, IW, M, KH, KW, stride, pad)
        need_d = _needs_scales(1, dg_dims) if ctx.needs_input_grad[0] else 0
        need_w = _needs_scales(4, (N, C, IH, IW, M, KH, KW, stride, pad), reflect) if ctx.needs_input_grad[1] else 0
        sdy = absmax_slot(dy) if (need_d or need_w) else None
        res = ctx.link.pop("dres", None) if ctx.link is not None else None
        if res is not None and not ctx.needs_input_grad[0]:
            raise _lib.KernelError("a residual link left a skip gradient for a convolution whose input needs no gradient")
        if ctx.needs_input_grad[0]:
            sd = sdy if need_d else None
            if res is not None:
                res = _c(res)
            if reflect:
                dxp = torch.empty((N, C, IH + 2 * pad, IW + 2 * pad), dtype=torch.float32, device=x.device)
                wp, wst, ent = _wpack(ctx.w_ref, 1, (N, C, IH + 2 * pad, IW + 2 * pad, M, KH, KW, stride, 0))
                _gather_workspace(x.device, 1, dg_dims)
                _conv_call("conv2d_dgrad", (ptr(dy), ptr(w), ptr(dxp), N, C, IH + 2 * pad, IW + 2 * pad, M, KH, KW, stride, 0, ptr(wp), wst,
                                            conv_precision, st), sd)
                _packed(ent, wst)
                dx = torch.empty_like(x)
                call("reflect_pad_bwd", ptr(dxp), ptr(dx), N * C, IH, IW, pad, st)
                if res is not None:
                    call("axpby", ptr(dx), ptr(res), ptr(dx), dx.numel(), 1.0, 1.0, st)
            else:
                dx = torch.empty_like(x)
                wp, wst, ent = _wpack(ctx.w_ref, 1, (N, C, IH, IW, M, KH, KW, stride, pad))
                _gather_workspace(x.device, 1, dg_dims)
                _conv_call("conv2d_dgrad", (ptr(dy), ptr(w), ptr(dx), N, C, IH, IW, M, KH, KW, stride, pad, ptr(wp), wst, conv_precision, st), sd, None, res)
                _packed(ent, wst)
        if ctx.needs_input_grad[1]:
            tgt = _grad_target(ctx.w_ref)
            if tgt is None:
                dw = torch.empty_like(w)
            prec = conv_precision
            sx = None
            if need_w:
                sx = ctx.sx if ctx.sx is not None else absmax_slot(x)
            elif prec == 3:
                prec = 0                               # a shape the split weight-gradient kernels leave to the exact-f32 ones: no slots
            sdw = sdy if need_w else None

            def wgrad(s, out, accumulate):
                _wgrad_workspace(x.device, C, M, KH, KW, stride, prec)
                _conv_call("conv2d_wgrad", (ptr(x), ptr(dy), ptr(out), N, C, IH, IW, M, KH, KW, stride, pad, reflect, accumulate, prec, s), sx, sdw)
            if tgt is not None:
                _enqueue_wgrad(lambda s: wgrad(s, tgt, 1), x, dy, sx, sdw)
            else:
                wgrad(st, dw, 0)
        if ctx.b_ref is not None and ctx.needs_input_grad[2]:
            tb = _grad_target(ctx.b_ref)
            if tb is not None:
                _enqueue_wgrad(lambda s: call("channel_sum", ptr(dy), ptr(tb), N, M, dy.shape[2] * dy.shape[3], 1, s), dy)
            else:
                db = torch.empty(M, dtype=torch.float32, device=x.device)
                call("channel_sum", ptr(dy), ptr(db), N, M, dy.shape[2] * dy.shape[3], 0, st)
        return dx, dw, db, None, None, None, None, None, None


def conv2d(x, w, bias=None, stride=1, pad=0, reflect=False, act=None, slope=0.2, link=None):
    return _Conv2d.apply(x, w, bias, int(stride), int(pad), 1 if reflect else 0, *_act_args(act, slope), link)


class _ConvTranspose2d(Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, out_pad, act, slope):
        x, w = _c(x), _c(w)
        N, C, IH, IW = x.shape
        Cw, M, KH, KW = w.shape
        if Cw != C:
            raise _lib.KernelError("conv_transpose2d: input has %d channels, weight expects %d" % (C, Cw))
        OH, OW = (IH - 1) * stride - 2 * pad + KH + out_pad, (IW - 1) * stride - 2 * pad + KW + out_pad
        y = torch.empty((N, M, OH, OW), dtype=torch.float32, device=x.device)
        wp, wst, ent = _wpack(w, 2, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad)
        sx = absmax_slot(x) if _needs_scales(2, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad) else None
        ctx.sx = sx
        _gather_workspace(x.device, 2, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad)
        _conv_call("conv_transpose2d_fwd", (ptr(x), ptr(w), ptr(bias), ptr(y), N, C, IH, IW, M, KH, KW, stride, pad, out_pad, act, slope,
                                            ptr(wp), wst, conv_precision | (NO_SPLIT_K if reproducible_forward else 0), stream_ptr()), sx)
        _packed(ent, wst)
        ctx.save_for_backward(x, w, y if act else None)
        ctx.w_ref, ctx.b_ref = w, bias
        ctx.cfg = (stride, pad, out_pad, act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, out_pad, act, slope = ctx.cfg
        dy = _c(dy)
        st = stream_ptr()
        N, C, IH, IW = x.shape
        _, M, KH, KW = w.shape
        if act:
            g = torch.empty_like(dy)
            call("act_bwd", ptr(dy), ptr(y), ptr(g), dy.numel(), act, slope, st)
            dy = g
        dx = dw = db = None
        need_d = _needs_scales(3, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad) if ctx.needs_input_grad[0] else 0
        need_w = _needs_scales(5, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad) if ctx.needs_input_grad[1] else 0
        sdy = absmax_slot(dy) if (need_d or need_w) else None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            wp, wst, ent = _wpack(ctx.w_ref, 3, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad)
            _gather_workspace(x.device, 3, (N, C, IH, IW, M, KH, KW, stride, pad), 0, out_pad)
            _conv_call("conv_transpose2d_dgrad", (ptr(dy), ptr(w), ptr(dx), N, C, IH, IW, M, KH, KW, stride, pad, out_pad, ptr(wp), wst,
                                                  conv_precision, st), sdy if need_d else None)
            _packed(ent, wst)
        if ctx.needs_input_grad[1]:
            tgt = _grad_target(ctx.w_ref)
            if tgt is None:
                dw = torch.empty_like(w)
            prec = conv_precision
            sx = None
            if need_w:
                sx = ctx.sx if ctx.sx is not None else absmax_slot(x)
            elif prec == 3:
                prec = 0
            sdw = sdy if need_w else None

            def wgrad(s, out, accumulate):
                _wgrad_workspace(x.device, M, C, KH, KW, stride, prec)     # (the kernel sees x and dy swapped)
                _conv_call("conv_transpose2d_wgrad", (ptr(x), ptr(dy), ptr(out), N, C, IH, IW, M, KH, KW, stride, pad, out_pad, accumulate, prec, s),
                           sx, sdw)
            if tgt is not None:
                _enqueue_wgrad(lambda s: wgrad(s, tgt, 1), x, dy, sx, sdw)
            else:
                wgrad(st, dw, 0)
        if ctx.b_ref is not None and ctx.needs_input_grad[2]:
            tb = _grad_target(ctx.b_ref)
            if tb is not None:
                _enqueue_wgrad(lambda s: call("channel_sum", ptr(dy), ptr(tb), N, M, dy.shape[2] * dy.shape[3], 1, s), dy)
            else:
                db = torch.empty(M, dtype=torch.float32, device=x.device)
                call("channel_sum", ptr(dy), ptr(db), N, M, dy.shape[2] * dy.shape[3], 0, st)
        return dx, dw, db, None, None, None, None, None


def conv_transpose2d(x, w, bias=None, stride=1, pad=0, out_pad=0, act=None, slope=0.2):
    return _ConvTranspose2d.apply(x, w, bias, int(stride), int(pad), int(out_pad), *_act_args(act, slope))


# ----------------------------------------------------------------------------------------
# BatchNorm2d (training statistics) + activation + residual
# ----------------------------------------------------------------------------------------
class _BatchNormTrain(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, momentum, eps, act, slope, link=None):
        ctx.link = link
        x = _c(x)
        N, C, H, W = x.shape
        if N * H * W <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
        if residual is not None:
            residual = _c(residual)
        y = torch.empty_like(x)
        stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
        ws = _lib.workspace(x.device, C * 128)
        sp = stats.data_ptr()                   # (row views cost ~3 us each on the host: 243 calls per step)
        slot = _producer_slot(x, C, H, W)       # f16x2: the output's largest magnitude comes out of this kernel's store loop
        _producer_call("batchnorm_train_fwd", (ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), sp, sp + 4 * C,
                                               ptr(running_mean), ptr(running_var), N, C, H * W, eps, momentum, act, slope, ptr(ws), stream_ptr()), slot)
        # the backward takes the ReLU / LeakyReLU mask from x when there was no residual (faoctasr.h): y is then not kept by this node
        need_y = act == ACT_TANH or (act and residual is not None)
        ctx.save_for_backward(x, gamma, stats, y if need_y else None, beta if (act and not need_y) else None)
        ctx.g_ref, ctx.b_ref = gamma, beta
        ctx.cfg = (act, slope, residual is not None)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)          # no zero-filled gradient tensor for `stats` on every backward
        _tag_absmax(y, slot)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, gamma, stats, y, beta = ctx.saved_tensors
        act, slope, has_res = ctx.cfg
        dy = _c(dy)
        N, C, H, W = x.shape
        dx = torch.empty_like(x)
        need_affine = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        tg = tb = dgamma = dbeta = None
        accumulate = 0
        if need_affine:
            tg, tb = _grad_target(ctx.g_ref), _grad_target(ctx.b_ref)
            if tg is not None and tb is not None:
                accumulate = 1
            else:
                tg = tb = None
                dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
                dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        dres = None
        if has_res and ctx.needs_input_grad[3]:
            dres = torch.empty_like(x) if act else dy
        ws = _lib.workspace(x.device, C * 128)
        sp = stats.data_ptr()
        slot = _producer_slot(x, C, H, W)       # f16x2: dx is the dY of the convolution in front of this layer
        _producer_call("batchnorm_train_bwd", (ptr(x), ptr(dy), ptr(y), ptr(gamma), ptr(beta), sp, sp + 4 * C, ptr(dx),
                                               ptr(tg if accumulate else dgamma), ptr(tb if accumulate else dbeta),
                                               ptr(dres) if (dres is not None and act) else None,
                                               N, C, H * W, act, slope, accumulate, ptr(ws), stream_ptr()), slot)
        _tag_absmax(dx, slot)
        if ctx.link is not None and dres is not None:
            ctx.link["dres"] = dres          # the block's first convolution adds it to its input gradient in its own epilogue
            dres = None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None


class _BatchNormEval(Function):
    """Inference-mode BatchNorm2d (running statistics): y = act(gamma * (x - mean) / sqrt(var + eps) + beta)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, act, slope):
        x = _c(x)
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        call("batchnorm_eval_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(y), N, C, H * W, eps, act, slope,
             stream_ptr())
        ctx.save_for_backward(gamma, running_var, y if act else None)
        ctx.cfg = (eps, act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        gamma, rv, y = ctx.saved_tensors
        eps, act, slope = ctx.cfg
        dy = _c(dy)
        N, C, H, W = dy.shape
        dx = torch.empty_like(dy)
        call("batchnorm_eval_bwd", ptr(dy), ptr(y), ptr(gamma), ptr(rv), ptr(dx), N, C, H * W, eps, act, slope, stream_ptr())
        return dx, None, None, None, None, None, None, None


def batchnorm_eval(x, gamma, beta, running_mean, running_var, eps=1e-5, act=None, slope=0.2):
    return _BatchNormEval.apply(x, gamma, beta, running_mean, running_var, float(eps), *_act_args(act, slope))


def batchnorm_train(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=None, slope=0.2, residual=None, link=None):
    y, _ = _BatchNormTrain.apply(x, gamma, beta, residual, running_mean, running_var, float(momentum), float(eps), *_act_args(act, slope),
                                 link if residual is not None else None)
    return y


class _InstanceNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, slope):
        x = _c(x)
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((2, N * C), dtype=torch.float32, device=x.device)
        ws = _lib.workspace(x.device, N * C * 128)
        call("instancenorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(stats[0]), ptr(stats[1]), N, C, H * W, eps, act, slope,
             ptr(ws), stream_ptr())
        ctx.save_for_backward(x, gamma, stats, y if act == ACT_TANH else None, beta if act and act != ACT_TANH else None)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats, y, beta = ctx.saved_tensors
        act, slope = ctx.cfg
        dy = _c(dy)
        N, C, H, W = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if gamma is not None else None
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if gamma is not None else None
        ws = _lib.workspace(x.device, N * C * 128)
        call("instancenorm_bwd", ptr(x), ptr(dy), ptr(y), ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), ptr(dx), ptr(dgamma), ptr(dbeta),
             N, C, H * W, act, slope, ptr(ws), stream_ptr())
        return dx, dgamma, dbeta, None, None, None


def instance_norm(x, gamma=None, beta=None, eps=1e-5, act=None, slope=0.2):
    return _InstanceNorm.apply(x, gamma, beta, float(eps), *_act_args(act, slope))


# ----------------------------------------------------------------------------------------
# pointwise
# ----------------------------------------------------------------------------------------
class _Act(Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        x = _c(x)
        y = torch.empty_like(x)
        call("act_fwd", ptr(x), ptr(y), x.numel(), act, slope, stream_ptr())
        ctx.save_for_backward(y)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(dy)
        call("act_bwd", ptr(dy), ptr(y), ptr(dx), dy.numel(), ctx.cfg[0], ctx.cfg[1], stream_ptr())
        return dx, None, None


def activation(x, act, slope=0.2):
    return _Act.apply(x, *_act_args(act, slope))


class _Cat2Act(Function):
    @staticmethod
    def forward(ctx, a, b, act, slope):
        if a.dim() != 4 or b.dim() != 4 or a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
            raise _lib.KernelError("cat2_act operands must be (N,C,H,W) tensors that agree in N, H and W: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        a, b = _c(a), _c(b)
        N, Ca, H, W = a.shape
        Cb = b.shape[1]
        y = torch.empty((N, Ca + Cb, H, W), dtype=torch.float32, device=a.device)
        slot = _producer_slot(a, Ca + Cb, H, W)
        _producer_call("cat2_act_fwd", (ptr(a), ptr(b), ptr(y), N, Ca, Cb, H * W, act, slope, stream_ptr()), slot)
        _tag_absmax(y, slot)
        ctx.save_for_backward(y if act else None)
        ctx.cfg = (act, slope, Ca, Cb)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        act, slope, Ca, Cb = ctx.cfg
        dy = _c(dy)
        N, _, H, W = dy.shape
        da = torch.empty((N, Ca, H, W), dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
        db = torch.empty((N, Cb, H, W), dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[1] else None
        call("cat2_act_bwd", ptr(dy), ptr(y), ptr(da), ptr(db), N, Ca, Cb, H * W, act, slope, stream_ptr())
        return da, db, None, None


def cat2_act(a, b, act=None, slope=0.2):
    """torch.cat([a, b], 1) followed by an activation (model.py:266+249, 268+431, 298+431)."""
    return _Cat2Act.apply(a, b, *_act_args(act, slope))


class _Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        _same_shape("add", a, b)
        a, b = _c(a), _c(b)
        y = torch.empty_like(a)
        call("axpby", ptr(a), ptr(b), ptr(y), a.numel(), 1.0, 1.0, stream_ptr())
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return _Add.apply(a, b)


class _Axpby(Function):
    @staticmethod
    def forward(ctx, a, b, alpha, beta):
        _same_shape("axpby", a, b)
        a, b = _c(a), _c(b)
        y = torch.empty_like(a)
        call("axpby", ptr(a), ptr(b), ptr(y), a.numel(), alpha, beta, stream_ptr())
        ctx.cfg = (alpha, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        alpha, beta = ctx.cfg
        dy = _c(dy)
        st = stream_ptr()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(dy)
            call("axpby", ptr(dy), ptr(dy), ptr(da), dy.numel(), alpha, 0.0, st)
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(dy)
            call("axpby", ptr(dy), ptr(dy), ptr(db), dy.numel(), beta, 0.0, st)
        return da, db, None, None


def axpby(a, b, alpha, beta):
    return _Axpby.apply(a, b, float(alpha), float(beta))


# ----------------------------------------------------------------------------------------
# Haar DWT
# ----------------------------------------------------------------------------------------
class _HaarAFB2D(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        N, C, H, W = x.shape
        ll = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
        hi = torch.empty((N, C, 3, H // 2, W // 2), dtype=torch.float32, device=x.device)
        call("haar_dwt2d_fwd", ptr(x), ptr(ll), ptr(hi), N * C, H, W, stream_ptr())
        ctx.shape = (N, C, H, W)
        return ll, hi

    @staticmethod
    def backward(ctx, dll, dhi):
        N, C, H, W = ctx.shape
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=(dll if dll is not None else dhi).device)
        call("haar_dwt2d_bwd", ptr(_c(dll)) if dll is not None else None, ptr(_c(dhi)) if dhi is not None else None, ptr(dx), N * C, H, W,
             stream_ptr())
        return dx


class _HaarSFB2D(Function):
    @staticmethod
    def forward(ctx, ll, hi):
        ll, hi = _c(ll), _c(hi)
        N, C, h, w = ll.shape
        x = torch.empty((N, C, 2 * h, 2 * w), dtype=torch.float32, device=ll.device)
        call("haar_dwt2d_bwd", ptr(ll), ptr(hi), ptr(x), N * C, 2 * h, 2 * w, stream_ptr())
        return x

    @staticmethod
    def backward(ctx, dx):
        dx = _c(dx)
        N, C, H, W = dx.shape
        dll = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=dx.device)
        dhi = torch.empty((N, C, 3, H // 2, W // 2), dtype=torch.float32, device=dx.device)
        call("haar_dwt2d_fwd", ptr(dx), ptr(dll), ptr(dhi), N * C, H, W, stream_ptr())
        return dll, dhi


def haar_afb2d(x):
    return _HaarAFB2D.apply(x)


def haar_sfb2d(ll, hi):
    return _HaarSFB2D.apply(ll, hi)


# ----------------------------------------------------------------------------------------
# general filter-bank DWT (csrc/dwt.hip): any even tap count up to 16, five padding modes, any size
# ----------------------------------------------------------------------------------------
DWT_MAX_TAPS = 16
DWT_MODES = (0, 1, 2, 4, 6)             # zero, symmetric, periodization, reflect, periodic (wavelets.mode_to_int)
_tap_arrays = {}


def host_taps(t):
    """The taps of a filter as a tuple of Python floats.  A tensor is read once (a device tensor: one synchronising copy) and
    the tuple cached on the tensor object for as long as its version counter stands, so that later calls -- those of a graph
    capture among them -- touch no device memory: the kernels take their taps by value.  Two consequences: the FIRST call on a
    device tensor must not fall inside a graph capture (``GraphedTrainStep`` warms up eagerly before it captures; anything else
    that captures calls the module once beforehand), and a write that does not bump the version counter (through ``.data``) is
    not seen -- assign a new tensor or use ``copy_`` to change taps."""
    if not isinstance(t, torch.Tensor):
        return tuple(float(v) for v in t)
    c = getattr(t, "_fa_taps", None)
    if c is not None and c[0] == t._version:
        return c[1]
    vals = tuple(t.detach().reshape(-1).to(torch.float32).tolist())
    t._fa_taps = (t._version, vals)
    return vals


def prime_taps(t, vals):
    """Record ``vals`` as the taps of tensor ``t`` without reading it (its owner knows them), unless a record stands."""
    c = getattr(t, "_fa_taps", None)
    if c is None or c[0] != t._version:
        t._fa_taps = (t._version, tuple(float(v) for v in vals))


def _tap_array(vals):
    a = _tap_arrays.get(vals)
    if a is None:
        if len(_tap_arrays) > 256:
            _tap_arrays.clear()
        a = _tap_arrays[vals] = (ctypes.c_float * len(vals))(*vals)
    return ctypes.cast(a, ctypes.c_void_p)


def dwt_bank(lo_w, hi_w, lo_h, hi_h):
    """Validate one level's filter bank -- the W-axis pair first, as AFB2D / SFB2D receive them -- and return it as host tuples."""
    bank = tuple(host_taps(t) for t in (lo_w, hi_w, lo_h, hi_h))
    for lo, hi in (bank[:2], bank[2:]):
        if len(lo) != len(hi):
            raise ValueError("lowpass and highpass filters must have the same length, got %d and %d" % (len(lo), len(hi)))
        if len(lo) % 2 or not 2 <= len(lo) <= DWT_MAX_TAPS:
            raise ValueError("filter length %d: the filter banks take an even number of taps, 2 to %d (pad an odd-length filter with "
                             "a zero tap)" % (len(lo), DWT_MAX_TAPS))
    return bank


def dwt_out_size(n, L, mode):
    """pywt.dwt_coeff_len as the reference uses it (lowlevel.py:134-153)."""
    return (n + 1) // 2 if mode == 2 else (n + L - 1) // 2


def _dwt_analysis(x, bank, mode):
    N, C, H, W = x.shape
    Lw, Lh = len(bank[0]), len(bank[2])
    if mode not in DWT_MODES:
        raise NotImplementedError("padding mode %d is not built (zero, symmetric, reflect, periodic, periodization are)" % mode)
    if H < Lh // 2 + 1 or W < Lw // 2 + 1:
        raise ValueError("a %d x %d image is below the minimum side L/2 + 1 of a %d (H) x %d (W) tap bank" % (H, W, Lh, Lw))
    x = _c(x)
    oh, ow = dwt_out_size(H, Lh, mode), dwt_out_size(W, Lw, mode)
    ll = torch.empty((N, C, oh, ow), dtype=torch.float32, device=x.device)
    hi = torch.empty((N, C, 3, oh, ow), dtype=torch.float32, device=x.device)
    call("dwt2d_analysis", ptr(x), ptr(ll), ptr(hi), N * C, H, W, _tap_array(bank[2]), _tap_array(bank[3]), Lh,
         _tap_array(bank[0]), _tap_array(bank[1]), Lw, mode, stream_ptr())
    return ll, hi


def _dwt_synthesis(ll, hi, bank, mode, crop=None):
    ref = ll if ll is not None else hi
    N, C = ref.shape[0], ref.shape[1]
    nh, nw = ref.shape[-2], ref.shape[-1]
    if ll is not None and hi is not None and (tuple(hi.shape) != (N, C, 3, nh, nw)):
        raise ValueError("lowpass %s and highpass %s coefficients do not belong together" % (tuple(ll.shape), tuple(hi.shape)))
    Lw, Lh = len(bank[0]), len(bank[2])
    if mode not in DWT_MODES:
        raise NotImplementedError("padding mode %d is not built (zero, symmetric, reflect, periodic, periodization are)" % mode)
    per = mode == 2
    if nh < ((Lh + 3) // 4 if per else Lh // 2) or nw < ((Lw + 3) // 4 if per else Lw // 2):
        raise ValueError("%d x %d coefficients are below the minimum side of a %d (H) x %d (W) tap bank" % (nh, nw, Lh, Lw))
    fh, fw = (2 * nh, 2 * nw) if per else (2 * nh - Lh + 2, 2 * nw - Lw + 2)
    oh, ow = (fh, fw) if crop is None else (min(fh, crop[0]), min(fw, crop[1]))
    ll = _c(ll) if ll is not None else None
    hi = _c(hi) if hi is not None else None
    y = torch.empty((N, C, oh, ow), dtype=torch.float32, device=ref.device)
    call("dwt2d_synthesis", ptr(ll), ptr(hi), ptr(y), N * C, nh, nw, oh, ow, _tap_array(bank[2]), _tap_array(bank[3]), Lh,
         _tap_array(bank[0]), _tap_array(bank[1]), Lw, mode, stream_ptr())
    return y


class _AFB2D(Function):
    """One analysis level (lowlevel.py:312-365).  ``bank`` = (lo_w, hi_w, lo_h, hi_h) host tuples, correlation kernels.  The
    backward is the reference's own: the synthesis bank run on the ANALYSIS taps, cropped to the input's size -- the adjoint for
    zero padding (and for periodization at even sizes), not for the folding and wrapping modes."""

    @staticmethod
    def forward(ctx, x, bank, mode):
        ctx.cfg = (bank, mode, x.shape[-2], x.shape[-1])
        return _dwt_analysis(x, bank, mode)

    @staticmethod
    def backward(ctx, dll, dhi):
        bank, mode, H, W = ctx.cfg
        return _dwt_synthesis(dll, dhi, bank, mode, crop=(H, W)), None, None


class _SFB2D(Function):
    """One synthesis level (lowlevel.py:647-694); the backward is the analysis bank run on the SYNTHESIS taps with the mode's
    padding, as the reference defines it."""

    @staticmethod
    def forward(ctx, ll, hi, bank, mode):
        ctx.cfg = (bank, mode, ll is not None, hi is not None)
        return _dwt_synthesis(ll, hi, bank, mode)

    @staticmethod
    def backward(ctx, dy):
        bank, mode, has_ll, has_hi = ctx.cfg
        dll, dhi = _dwt_analysis(dy, bank, mode)
        return dll if has_ll else None, dhi if has_hi else None, None, None


def afb2d(x, lo_w, hi_w, lo_h, hi_h, mode):
    """(ll, hi) of one analysis level; the filters are tensors or sequences, W-axis pair first, in correlation order."""
    return _AFB2D.apply(x, dwt_bank(lo_w, hi_w, lo_h, hi_h), int(mode))


def sfb2d(ll, hi, lo_w, hi_w, lo_h, hi_h, mode):
    """One synthesis level; ``hi`` (or ``ll``) may be None for zeros."""
    return _SFB2D.apply(ll, hi, dwt_bank(lo_w, hi_w, lo_h, hi_h), int(mode))


# ----------------------------------------------------------------------------------------
# 1-D filter-bank DWT over rows (csrc/dwt1d.hip): all J levels of a row in one launch, rows up to DWT1D_FUSED_MAX samples in LDS
# ----------------------------------------------------------------------------------------
DWT1D_FUSED_MAX = 8192                  # csrc/dwt1d.hip DWT1D_FUSED_MAX (faoctasr_dwt1d_fused_max)
DWT1D_MAX_LEVELS = 8


def dwt1d_bank(lo, hi):
    """Validate one 1-D filter pair and return it as host tuples."""
    return dwt_bank(lo, hi, lo, hi)[:2]


def dwt1d_lengths(n, L, mode, J):
    """[n_0 .. n_J]: the input length of every analysis level and the coarsest output, n_(j+1) = dwt_out_size(n_j)."""
    out = [int(n)]
    for _ in range(J):
        out.append(dwt_out_size(out[-1], L, mode))
    return out


def dwt1d_inverse_lengths(lo_len, hi_lens, L, mode):
    """The inverse's length bookkeeping, coarsest level first as ``DWT1DInverse`` walks them.  ``hi_lens[j]`` is the length of
    level j's highpass (0 = finest), None for a missing level.  -> (counts, fulls): per level j the coefficient count the level
    runs on -- the running lowpass after a surplus last sample was dropped -- and the length of its result, ``2 c - L + 2``
    (periodization: ``2 c``).  A lowpass that still differs from its level's highpass raises ``ValueError``."""
    J = len(hi_lens)
    counts, fulls = [0] * J, [0] * J
    m = int(lo_len)
    for j in reversed(range(J)):
        c = hi_lens[j]
        if c is not None:
            if m == c + 1:
                m = c
            elif m != c:
                raise ValueError("level %d: a lowpass of %d samples does not belong to a highpass of %d (one surplus sample is dropped, no more)" % (j, m, c))
        if m < ((L + 3) // 4 if mode == 2 else L // 2):
            raise ValueError("level %d: %d coefficients are below the minimum of a %d tap bank" % (j, m, L))
        counts[j] = m
        m = fulls[j] = 2 * m if mode == 2 else 2 * m - L + 2
    return counts, fulls


def _rows(t):
    """(tensor, (inner, outer stride, row stride)) of an (N, C, n) operand whose samples are contiguous, else of its contiguous copy."""
    N, C, n = t.shape
    s = t.stride()
    if t.is_cuda and t.dtype == torch.float32 and (s[2] == 1 or n == 1) and s[1] >= n and s[0] >= 0:
        return t, (C, s[0], s[1])
    t = _c(t)
    return t, (C, C * n, n)


def _dwt1d_check(bank, mode, J):
    if mode not in DWT_MODES:
        raise NotImplementedError("padding mode %d is not built (zero, symmetric, reflect, periodic, periodization are)" % mode)
    if not 1 <= J <= DWT1D_MAX_LEVELS:
        raise ValueError("the 1-D transform runs J = 1..%d levels, got %d" % (DWT1D_MAX_LEVELS, J))


def _dwt1d_fused(n, fused):
    if fused is None:
        return n <= DWT1D_FUSED_MAX
    if fused and n > DWT1D_FUSED_MAX:
        raise ValueError("a row of %d samples is beyond the fused launch's limit DWT1D_FUSED_MAX = %d" % (n, DWT1D_FUSED_MAX))
    return bool(fused)


def _dwt1d_analysis(x, bank, mode, in_lens, fused):
    """The analysis launch(es): x (N, C, n) -> (lo, [hi_0 .. hi_(J-1)]); ``in_lens[j]`` the length level j reads (what its source
    holds or one zero more).  One call fused, one per level tiled (the lowpass then travels through device memory)."""
    N, C, n = x.shape
    J, L = len(in_lens), len(bank[0])
    outs = [dwt_out_size(m, L, mode) for m in in_lens]
    his = [torch.empty((N, C, o), dtype=torch.float32, device=x.device) for o in outs]
    x, (inner, so, sr) = _rows(x)
    h0, h1 = _tap_array(bank[0]), _tap_array(bank[1])
    if fused:
        lo = torch.empty((N, C, outs[-1]), dtype=torch.float32, device=x.device)
        hp = (ctypes.c_void_p * J)(*[ptr(h) for h in his])
        ln = (ctypes.c_int * J)(*in_lens)
        call("dwt1d_analysis", x.data_ptr(), inner, so, sr, ptr(lo), ctypes.cast(hp, ctypes.c_void_p), N * C, n,
             ctypes.cast(ln, ctypes.c_void_p), J, h0, h1, L, mode, 1, stream_ptr())
        return lo, his
    lo = x
    for j in range(J):
        src, (inner, so, sr) = _rows(lo)
        lo = torch.empty((N, C, outs[j]), dtype=torch.float32, device=x.device)
        hp = (ctypes.c_void_p * 1)(ptr(his[j]))
        ln = (ctypes.c_int * 1)(in_lens[j])
        call("dwt1d_analysis", src.data_ptr(), inner, so, sr, ptr(lo), ctypes.cast(hp, ctypes.c_void_p), N * C, src.shape[-1],
             ctypes.cast(ln, ctypes.c_void_p), 1, h0, h1, L, mode, 0, stream_ptr())
    return lo, his


def _dwt1d_synthesis(lo, his, bank, mode, counts, crops, fused):
    """The synthesis launch(es): lo (N, C, >= counts[-1]), his[j] (N, C, counts[j]) or None -> y (N, C, crops[0]); level j's result
    is cropped to ``crops[j]`` (``crops[j] == counts[j - 1]`` for j > 0)."""
    N, C = lo.shape[0], lo.shape[1]
    J, L = len(counts), len(bank[0])
    his = [_c(h) if h is not None else None for h in his]
    g0, g1 = _tap_array(bank[0]), _tap_array(bank[1])
    lo, (inner, so, sr) = _rows(lo)
    if fused:
        y = torch.empty((N, C, crops[0]), dtype=torch.float32, device=lo.device)
        hp = (ctypes.c_void_p * J)(*[ptr(h) for h in his])
        cn = (ctypes.c_int * J)(*counts)
        call("dwt1d_synthesis", lo.data_ptr(), inner, so, sr, ctypes.cast(hp, ctypes.c_void_p), ptr(y), N * C, ctypes.cast(cn, ctypes.c_void_p), J,
             crops[0], g0, g1, L, mode, 1, stream_ptr())
        return y
    for j in reversed(range(J)):
        y = torch.empty((N, C, crops[j]), dtype=torch.float32, device=lo.device)
        hp = (ctypes.c_void_p * 1)(ptr(his[j]))
        cn = (ctypes.c_int * 1)(counts[j])
        call("dwt1d_synthesis", lo.data_ptr(), inner, so, sr, ctypes.cast(hp, ctypes.c_void_p), ptr(y), N * C, ctypes.cast(cn, ctypes.c_void_p), 1,
             crops[j], g0, g1, L, mode, 0, stream_ptr())
        lo, (inner, so, sr) = _rows(y)
    return y


def _dev_rows(t, what):
    if t.dim() != 3:
        raise ValueError("%s: the 1-D transform takes (N, C, L) tensors, got %d dimensions" % (what, t.dim()))
    if not (t.is_cuda and t.dtype == torch.float32):
        raise _lib.KernelError("kernel operand must be an fp32 device tensor, got %s %s on %s" % (tuple(t.shape), t.dtype, t.device))


class _DWT1DAnalysis(Function):
    """J analysis levels of (N, C, n) rows: ``apply(x, bank, mode, J, fused) -> (lo, hi_0, .., hi_(J-1))``, ``bank`` = (h0, h1) host
    tuples, correlation kernels.  The backward is the reference's own (lowlevel.py:401-424 per level): the synthesis bank on the
    ANALYSIS taps, every level cropped to the length its forward read -- one launch where the forward was one."""

    @staticmethod
    def forward(ctx, x, bank, mode, J, fused):
        _dwt1d_check(bank, mode, J)
        if x.dim() != 3:
            raise ValueError("the 1-D transform takes (N, C, L) tensors, got %d dimensions" % x.dim())
        L = len(bank[0])
        lens = dwt1d_lengths(x.shape[-1], L, mode, J)
        for j in range(J):
            if lens[j] < L // 2 + 1:
                raise ValueError("level %d would read %d samples, below the minimum length L/2 + 1 = %d of a %d tap bank" % (j, lens[j], L // 2 + 1, L))
        fused = _dwt1d_fused(lens[0], fused)
        _dev_rows(x, "dwt1d_analysis")
        ctx.cfg = (bank, mode, lens, fused)
        lo, his = _dwt1d_analysis(x, bank, mode, lens[:J], fused)
        return (lo,) + tuple(his)

    @staticmethod
    def backward(ctx, dlo, *dhis):
        bank, mode, lens, fused = ctx.cfg
        return _dwt1d_synthesis(dlo, list(dhis), bank, mode, lens[1:], lens[:-1], fused), None, None, None, None


class _DWT1DSynthesis(Function):
    """The inverse over all levels: ``apply(lo, bank, mode, fused, hi_0, .., hi_(J-1)) -> y``, a ``None`` level standing for zeros;
    a surplus last sample of the running lowpass is dropped between levels, as ``DWT1DInverse`` does.  The backward is the
    reference's (lowlevel.py:730-743 per level): the analysis bank on the SYNTHESIS taps with the mode's padding, a zero
    appended wherever the forward dropped a sample -- one launch where the forward was one."""

    @staticmethod
    def forward(ctx, lo, bank, mode, fused, *his):
        J = len(his)
        _dwt1d_check(bank, mode, J)
        for t in (lo,) + his:
            if t is not None and t.dim() != 3:
                raise ValueError("the 1-D transform takes (N, C, L) tensors, got %d dimensions" % t.dim())
        for j, h in enumerate(his):
            if h is not None and tuple(h.shape[:2]) != tuple(lo.shape[:2]):
                raise ValueError("level %d: highpass %s and lowpass %s do not belong together" % (j, tuple(h.shape), tuple(lo.shape)))
        counts, fulls = dwt1d_inverse_lengths(lo.shape[-1], [None if h is None else h.shape[-1] for h in his], len(bank[0]), mode)
        fused = _dwt1d_fused(fulls[0], fused)
        for t in (lo,) + his:
            if t is not None:
                _dev_rows(t, "dwt1d_synthesis")
        ctx.cfg = (bank, mode, counts, fulls, lo.shape[-1], tuple(h is not None for h in his), fused)
        return _dwt1d_synthesis(lo, list(his), bank, mode, counts, [fulls[0]] + counts[:-1], fused)

    @staticmethod
    def backward(ctx, dy):
        bank, mode, counts, fulls, lo_len, has, fused = ctx.cfg
        dlo, dhis = _dwt1d_analysis(dy, bank, mode, fulls, fused)
        if lo_len > counts[-1]:                 # the coarsest lowpass lost its last sample on the way in
            dlo = torch.nn.functional.pad(dlo, (0, lo_len - counts[-1]))
        return (dlo, None, None, None) + tuple(d if h else None for d, h in zip(dhis, has))


def dwt1d_analysis(x, h0, h1, mode, J=1, fused=None):
    """(lo, [hi_0 .. hi_(J-1)]) of J analysis levels of (N, C, n) rows in one launch; the filters are tensors or sequences in
    correlation order (the decomposition taps reversed).  ``fused``: None picks the fused launch up to ``DWT1D_FUSED_MAX``
    samples a row and the tiled one (a launch per level) beyond, True / False force one (True beyond the limit raises)."""
    out = _DWT1DAnalysis.apply(x, dwt1d_bank(h0, h1), int(mode), int(J), fused)
    return out[0], list(out[1:])


def dwt1d_synthesis(lo, highs, g0, g1, mode, fused=None):
    """The inverse of ``dwt1d_analysis``'s coefficients in one launch; a ``None`` entry of ``highs`` stands for zeros."""
    return _DWT1DSynthesis.apply(lo, dwt1d_bank(g0, g1), int(mode), fused, *highs)


def afb1d(x, h0, h1, mode):
    """(lo, hi) of one analysis level of (N, C, n) rows."""
    return _DWT1DAnalysis.apply(x, dwt1d_bank(h0, h1), int(mode), 1, None)


def sfb1d(lo, hi, g0, g1, mode):
    """One synthesis level of (N, C, n) coefficients; ``hi`` may be None for zeros."""
    return _DWT1DSynthesis.apply(lo, dwt1d_bank(g0, g1), int(mode), None, hi)


# ----------------------------------------------------------------------------------------
# stationary (a-trous) wavelet transform (csrc/swt.hip): any even tap count up to 16, four extensions, dilations 1..8
# ----------------------------------------------------------------------------------------
SWT_MODES = (0, 1, 4, 6)                # zero, symmetric, reflect, periodic (wavelets.swt_mode_to_int)
SWT_MAX_LEVELS = 4                      # dilation 2^(J-1) <= 8


def swt_bank(lo_h, hi_h, lo_w, hi_w):
    """Validate a stationary transform's bank -- the H-axis pair first, every filter in WAVELET order (dec_* / rec_* as given,
    not the reversed buffers) -- and return it as host tuples."""
    return dwt_bank(lo_h, hi_h, lo_w, hi_w)


def _swt_geometry(H, W, bank, J, mode):
    Lh, Lw = len(bank[0]), len(bank[2])
    if mode not in SWT_MODES:
        raise NotImplementedError("extension %d is not built for the stationary transform (zero, symmetric, reflect, periodic are)" % mode)
    if not 1 <= J <= SWT_MAX_LEVELS:
        raise ValueError("the stationary transform runs J = 1..%d levels (dilation up to %d), got %d" % (SWT_MAX_LEVELS, 1 << (SWT_MAX_LEVELS - 1), J))
    d = 1 << (J - 1)
    if H < Lh * d // 2 + 1 or W < Lw * d // 2 + 1:
        raise ValueError("a %d x %d image is below the minimum side L 2^(J-1) / 2 + 1 of a %d (H) x %d (W) tap bank at J = %d: %d x %d"
                         % (H, W, Lh, Lw, J, Lh * d // 2 + 1, Lw * d // 2 + 1))


def _plane_strided(t):
    """(tensor, plane stride) for an (N, C, H, W) operand whose planes are dense and evenly spaced -- band 0 of a level's
    (N, C, 4, H, W) output -- else a contiguous copy."""
    N, C, H, W = t.shape
    s = t.stride()
    if t.is_cuda and t.dtype == torch.float32 and s[3] == 1 and s[2] == W and s[1] >= H * W and (N == 1 or s[0] == C * s[1]):
        return t, s[1]
    return _c(t), H * W


def _swt_level(x, bank, d, mode, scale):
    """One analysis launch: planes of x (possibly band 0 of a previous level, read in place) -> (N, C, 4, H, W)."""
    N, C, H, W = x.shape
    x, ps = _plane_strided(x)
    y = torch.empty((N, C, 4, H, W), dtype=torch.float32, device=x.device)
    call("swt2d_analysis", ptr(x) if x.is_contiguous() else x.data_ptr(), ps, ptr(y), N * C, H, W, _tap_array(bank[0]), _tap_array(bank[1]), len(bank[0]),
         _tap_array(bank[2]), _tap_array(bank[3]), len(bank[2]), d, mode, scale, stream_ptr())
    return y


def _swt_level_adjoint(c, bank, d, mode, scale, band0=None, replace=False):
    """One adjoint launch: (N, C, 4, H, W) -> (N, C, H, W).  ``band0``, an (N, C, H, W) tensor, is added to band 0 of ``c`` as the
    kernel reads it, or read in its place (``replace``): the levels chain without a copy of ``c``."""
    N, C, _, H, W = c.shape
    c = _c(c)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=c.device)
    call("swt2d_adjoint", ptr(c), ptr(out), H * W, ptr(_c(band0)) if band0 is not None else None, H * W, int(replace), N * C, H, W,
         _tap_array(bank[0]), _tap_array(bank[1]), len(bank[0]), _tap_array(bank[2]), _tap_array(bank[3]), len(bank[2]), d, mode, scale,
         stream_ptr())
    return out


class _SWTAnalysis(Function):
    """J levels of the stationary transform: ``apply(x, bank, mode, J) -> J tensors (N, C, 4, H, W)``, level j at dilation 2^j on
    band 0 of level j - 1 (read in place).  ``bank`` = (lo_h, hi_h, lo_w, hi_w) host tuples in wavelet order.  The backward is
    the exact adjoint in every mode, coarse to fine: the gradient of a level joins band 0 of the next finer level's cotangent
    inside that level's launch (autograd hands a zero tensor for a level nothing depends on)."""

    @staticmethod
    def forward(ctx, x, bank, mode, J):
        _swt_geometry(x.shape[-2], x.shape[-1], bank, J, mode)
        ctx.cfg = (bank, mode, J)
        out, ll = [], x
        for j in range(J):
            y = _swt_level(ll, bank, 1 << j, mode, 1.0)
            out.append(y)
            ll = y[:, :, 0]
        return tuple(out)

    @staticmethod
    def backward(ctx, *dys):
        bank, mode, J = ctx.cfg
        g = None
        for j in reversed(range(J)):
            g = _swt_level_adjoint(dys[j], bank, 1 << j, mode, 1.0, band0=g)
        return g, None, None, None


class _SWTSynthesis(Function):
    """The periodic inverse: ``apply(bank, *coeffs) -> x`` for the list ``SWTForward`` returns, ``bank`` = (g0_h, g1_h, g0_w, g1_w)
    rec taps in wavelet order.  Coarse to fine; the coarsest level's band 0 and bands 1..3 of every level are used, the finer
    levels' band 0 is ignored: the kernel reads the coarser level's result in its place.  A level is the adjoint kernel on the
    reversed taps with scale 1/4 (1/2 per axis), its backward the analysis kernel on the same taps and scale."""

    @staticmethod
    def forward(ctx, bank, *coeffs):
        J = len(coeffs)
        N, C, four, H, W = coeffs[-1].shape
        if four != 4 or any(tuple(c.shape) != (N, C, 4, H, W) for c in coeffs):
            raise ValueError("the coefficients of a stationary transform are (N, C, 4, H, W) tensors of one shape, got %s" % [tuple(c.shape) for c in coeffs])
        _swt_geometry(H, W, bank, J, 6)
        rev = tuple(t[::-1] for t in bank)
        ctx.cfg = (rev, J)
        ll = None
        for j in reversed(range(J)):
            ll = _swt_level_adjoint(coeffs[j], rev, 1 << j, 6, 0.25, band0=ll, replace=True)
        return ll

    @staticmethod
    def backward(ctx, dy):
        rev, J = ctx.cfg
        grads, g = [], dy
        for j in range(J):
            G = _swt_level(g, rev, 1 << j, 6, 0.25)
            grads.append(G)
            g = G[:, :, 0]
        for G in grads[:-1]:                    # the finer levels' band 0 does not reach the result (read above, then cleared)
            G[:, :, 0].zero_()
        return (None,) + tuple(grads)


def swt_analysis(x, lo_h, hi_h, lo_w, hi_w, mode, J=1):
    """The J levels of the stationary transform of x, a tuple of (N, C, 4, H, W) tensors; the filters are tensors or sequences
    in wavelet order (dec_lo, dec_hi), the H-axis pair first; ``mode`` one of ``SWT_MODES``."""
    return _SWTAnalysis.apply(x, swt_bank(lo_h, hi_h, lo_w, hi_w), int(mode), int(J))


def swt_synthesis(coeffs, lo_h, hi_h, lo_w, hi_w):
    """The periodic inverse of ``swt_analysis``'s list; the filters are the rec taps in wavelet order, the H-axis pair first."""
    return _SWTSynthesis.apply(swt_bank(lo_h, hi_h, lo_w, hi_w), *coeffs)


# ----------------------------------------------------------------------------------------
# dual-tree complex wavelet transform (csrc/dtcwt.hip): one fused launch per level and direction
# ----------------------------------------------------------------------------------------
DTCWT_MAX_TAPS = 20                     # q-shift filters: even, 4..20; level-1 filters: odd, 3..19


def dtcwt_layout(o_dim, ri_dim):
    """The axis names ('n', 'c', 'h', 'w', 'o', 'r') of a bandpass tensor in the order ``o_dim`` / ``ri_dim`` put them, by the
    reference's own rule (transform_funcs.py:10-29): both taken modulo 6, the orientations stacked into the (N, C, H, W) band at
    ``o_dim`` (less one if ``ri_dim`` lies before it), then real and imaginary parts stacked at ``ri_dim``."""
    if o_dim == ri_dim:
        raise ValueError("Orientations and real/imaginary parts must be in different dimensions.")
    o, r = int(o_dim) % 6, int(ri_dim) % 6
    if r < o:
        o -= 1
    if o > 4:
        raise ValueError("o_dim %d with ri_dim %d puts the orientations past the last axis of the 5-d band" % (o_dim, ri_dim))
    names = ["n", "c", "h", "w"]
    names.insert(o, "o")
    names.insert(r, "r")
    return tuple(names)


def dtcwt_sizes(H, W, J):
    """Per level j = 0 .. J-1: ((input rows, cols) after the module's padding, (lowpass rows, cols), (bandpass rows, cols))."""
    out = []
    h, w = H + H % 2, W + W % 2
    out.append(((h, w), (h, w), (h // 2, w // 2)))
    for _ in range(1, J):
        h, w = (h if h % 4 == 0 else h + 2), (w if w % 4 == 0 else w + 2)
        out.append(((h, w), (h // 2, w // 2), (h // 4, w // 4)))
        h, w = h // 2, w // 2
    return out


def _dtcwt_taps1(f0, f1, f2=None):
    """The level-1 taps as host tuples: (f0, f1), or (f0, f1, f2) with the third (bandpass) filter of a three-filter bank."""
    f0, f1 = host_taps(f0), host_taps(f1)
    for f in (f0, f1):
        if len(f) % 2 == 0 or not 3 <= len(f) < DTCWT_MAX_TAPS:
            raise ValueError("filter length %d: the level-1 filters take an odd number of taps, 3 to %d" % (len(f), DTCWT_MAX_TAPS - 1))
    if f2 is None:
        return f0, f1
    f2 = host_taps(f2)
    if len(f2) % 2 == 0 or not 3 <= len(f2) < DTCWT_MAX_TAPS:
        raise ValueError("filter length %d: the third level-1 filter takes an odd number of taps, 3 to %d" % (len(f2), DTCWT_MAX_TAPS - 1))
    return f0, f1, f2


def _dtcwt_taps2(fa0, fb0, fa1, fb1, fa2=None, fb2=None):
    """The q-shift taps as host tuples: (a0, b0, a1, b1), or with the third pair of a three-filter bank (a0, b0, a1, b1, a2, b2)."""
    f = tuple(host_taps(t) for t in (fa0, fb0, fa1, fb1))
    if len(set(len(t) for t in f)) != 1:
        raise ValueError("the four q-shift filters must have the same length, got %s" % [len(t) for t in f])
    if len(f[0]) % 2 or not 4 <= len(f[0]) <= DTCWT_MAX_TAPS:
        raise ValueError("filter length %d: the q-shift filters take an even number of taps, 4 to %d" % (len(f[0]), DTCWT_MAX_TAPS))
    if fa2 is None and fb2 is None:
        return f
    if fa2 is None or fb2 is None:
        raise ValueError("the third q-shift filters come as a pair (tree a, tree b), got one of them")
    g = (host_taps(fa2), host_taps(fb2))
    if any(len(t) != len(f[0]) for t in g):
        raise ValueError("the third q-shift filters must have the length of the other four (%d), got %s" % (len(f[0]), [len(t) for t in g]))
    return f + g


def _taps1_args(taps):
    """(pointer, length) of the three level-1 filters, as the entry points take them: (NULL, 0) for the third of a two-filter bank."""
    return tuple(a for t in taps for a in (_tap_array(t), len(t))) + (None, 0) * (3 - len(taps))


def _taps2_args(taps):
    """The six q-shift tap pointers and their length, as the entry points take them: two NULLs for the third pair of a two-filter bank."""
    return tuple(_tap_array(t) for t in taps) + (None,) * (6 - len(taps)) + (len(taps[0]),)


def _dtcwt_dev(t, what):
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (what, t.dtype))
    if not t.is_cuda:
        raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))


def _dtcwt_low(t):
    """(tensor, n stride, c stride, row stride) of an (N, C, H, W) lowpass input with unit-stride columns, else of a copy."""
    if t.stride(3) != 1 and t.shape[3] > 1:
        t = t.contiguous()
    s = t.stride()
    return t, s[0], s[1], s[2]


def _dtcwt_high_strides(h, names):
    s = dict(zip(names, h.stride()))
    st = tuple(s[k] for k in "ncohwr")
    vec = int(st[5] == 1 and all(v % 2 == 0 for v in st[:5]) and h.data_ptr() % 8 == 0)
    return st, vec


def _dtcwt_check_high(h, names, rows, cols, N, C):
    if h.dim() != 6:
        raise ValueError("Bandpass inputs must have 6 dimensions, got %d" % h.dim())
    size = dict(zip(names, h.shape))
    if size["o"] != 6:
        raise ValueError("Inverse transform must have input with 6 orientations, got %d" % size["o"])
    if size["r"] != 2:
        raise ValueError("Inputs must be complex with real and imaginary parts in the ri dimension, got size %d" % size["r"])
    if rows is not None and (2 * size["h"], 2 * size["w"], size["n"], size["c"]) != (rows, cols, N, C):
        raise ValueError("the lowpass (%d, %d, %d, %d) must be twice the bandpass (%d, %d, %d, %d) in rows and columns"
                         % (N, C, rows, cols, size["n"], size["c"], size["h"], size["w"]))
    return size


def _dtcwt_forward(x, taps, level1, mode, names, want_ll=True, want_hi=True):
    """One analysis launch.  ``level1``: taps = (f0, f1), 'same' filters, x even-sided; else taps = (h0a, h0b, h1a, h1b) and x a
    multiple of 4 a side.  Returns (ll or None, highs or None)."""
    if x.dim() != 4:
        raise ValueError("the transform takes inputs of 4 dimensions (N, C, H, W), got %d" % x.dim())
    N, C, H, W = x.shape
    q = 2 if level1 else 4
    if H % q or W % q or H < q or W < q:
        raise ValueError("a level-%s input must have rows and columns that are a multiple of %d, got %d x %d" % ("1" if level1 else ">=2", q, H, W))
    _dtcwt_dev(x, "the input")
    x, sn, sc, sr = _dtcwt_low(x)
    lh, lw = (H, W) if level1 else (H // 2, W // 2)
    ll = torch.empty((N, C, lh, lw), dtype=torch.float32, device=x.device) if want_ll else None
    hi, st, vec = None, (0,) * 6, 0
    if want_hi:
        size = {"n": N, "c": C, "o": 6, "h": lh // 2, "w": lw // 2, "r": 2}
        hi = torch.empty(tuple(size[k] for k in names), dtype=torch.float32, device=x.device)
        st, vec = _dtcwt_high_strides(hi, names)
    if not want_hi:                         # the lowpass of a three-filter bank is the two-filter one: no third filter
        taps = taps[:2] if level1 else taps[:4]
    if level1:
        call("dtcwt_fwd_j1", x.data_ptr(), sn, sc, sr, ptr(ll), ptr(hi), *st, vec, N, C, H, W, *_taps1_args(taps), mode, stream_ptr())
    else:
        call("dtcwt_fwd_j2", x.data_ptr(), sn, sc, sr, ptr(ll), ptr(hi), *st, vec, N, C, H, W, *_taps2_args(taps), stream_ptr())
    return ll, hi


def _dtcwt_inverse(ll, hi, taps, level1, mode, names):
    """One synthesis launch; ``ll`` or ``hi`` may be None (zeros, not computed)."""
    if ll is None and hi is None:
        raise ValueError("the lowpass and the bandpass cannot both be missing")
    if ll is not None:
        if ll.dim() != 4:
            raise ValueError("the lowpass takes 4 dimensions (N, C, H, W), got %d" % ll.dim())
        N, C, R, Q = ll.shape
        if R % 2 or Q % 2 or R < 2 or Q < 2:
            raise ValueError("a lowpass must have rows and columns that are a multiple of 2, got %d x %d" % (R, Q))
        if hi is not None:
            _dtcwt_check_high(hi, names, R, Q, N, C)
    else:
        size = _dtcwt_check_high(hi, names, None, None, None, None)
        N, C, R, Q = size["n"], size["c"], 2 * size["h"], 2 * size["w"]
    for t, what in ((ll, "the lowpass"), (hi, "the bandpass")):
        if t is not None:
            _dtcwt_dev(t, what)
    dev = (ll if ll is not None else hi).device
    sn = sc = sr = 0
    if ll is not None:
        ll, sn, sc, sr = _dtcwt_low(ll)
    st = _dtcwt_high_strides(hi, names)[0] if hi is not None else (0,) * 6
    H, W = (R, Q) if level1 else (2 * R, 2 * Q)
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
    lp, hp = (ll.data_ptr() if ll is not None else None), (hi.data_ptr() if hi is not None else None)
    if level1:
        call("dtcwt_inv_j1", lp, sn, sc, sr, hp, *st, ptr(y), N, C, H, W, *_taps1_args(taps), mode, stream_ptr())
    else:
        call("dtcwt_inv_j2", lp, sn, sc, sr, hp, *st, ptr(y), N, C, H, W, *_taps2_args(taps), stream_ptr())
    return y


def _swap_ab(t):
    return (t[1], t[0], t[3], t[2]) + ((t[5], t[4]) if len(t) == 6 else ())


class _DTCWTFwd(Function):
    """One analysis level: ``apply(x, taps, level1, skip_hps, names, mode) -> (ll, highs)``; a skipped bandpass is a 0-d zero, as in
    the reference.  The backward is the reference's: the matching inverse on the same (analysis) taps, a and b swapped at levels
    >= 2 -- the exact adjoint.  A cotangent nothing depends on goes to the kernel as a null pointer."""

    @staticmethod
    def forward(ctx, x, taps, level1, skip_hps, names, mode):
        ctx.cfg = (taps if level1 else _swap_ab(taps), level1, mode, names)
        ctx.set_materialize_grads(False)
        ll, hi = _dtcwt_forward(x, taps, level1, mode, names, want_hi=not skip_hps)
        if skip_hps:
            hi = ll.new_zeros([])
            ctx.mark_non_differentiable(hi)
        return ll, hi

    @staticmethod
    def backward(ctx, dl, dh):
        taps, level1, mode, names = ctx.cfg
        if dh is not None and dh.dim() == 0:
            dh = None
        if dl is None and dh is None:
            return (None,) * 6
        return (_dtcwt_inverse(dl, dh, taps, level1, mode, names),) + (None,) * 5


class _DTCWTFwdJ1(_DTCWTFwd):
    """transform_funcs.py:343-374 FWD_J1 on csrc/dtcwt.hip (``level1`` = True)."""


class _DTCWTFwdJ2(_DTCWTFwd):
    """transform_funcs.py:377-413 FWD_J2PLUS (``level1`` = False; always the symmetric extension)."""


class _DTCWTInv(Function):
    """One synthesis level: ``apply(ll, highs, taps, level1, names, mode) -> y``; ``ll`` or ``highs`` may be None.  The backward is
    the matching forward on the same (synthesis) taps, a and b swapped at levels >= 2, and computes only the gradients asked for."""

    @staticmethod
    def forward(ctx, ll, hi, taps, level1, names, mode):
        ctx.cfg = (taps if level1 else _swap_ab(taps), level1, mode, names)
        return _dtcwt_inverse(ll, hi, taps, level1, mode, names)

    @staticmethod
    def backward(ctx, dy):
        taps, level1, mode, names = ctx.cfg
        want_ll, want_hi = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_ll or want_hi):
            return (None,) * 6
        dl, dh = _dtcwt_forward(dy, taps, level1, mode, names, want_ll=want_ll, want_hi=want_hi)
        return (dl, dh) + (None,) * 4


class _DTCWTInvJ1(_DTCWTInv):
    """transform_funcs.py:416-449 INV_J1."""


class _DTCWTInvJ2(_DTCWTInv):
    """transform_funcs.py:452-488 INV_J2PLUS."""


def dtcwt_fwd_j1(x, h0o, h1o, skip_hps=False, o_dim=2, ri_dim=-1, mode=1, h2o=None):
    """Level 1 of the forward transform: x (N, C, H, W), H and W even -> (ll (N, C, H, W), highs in the ``o_dim`` / ``ri_dim`` layout,
    default (N, C, 6, H/2, W/2, 2)).  The filters are tensors or sequences as the modules register them (taps reversed).
    ``mode`` 1 is the symmetric extension, any other ``wavelets.mode_to_int`` code pads with zeros, as the reference does.
    ``h2o``: the bandpass filter of a three-filter bank (fwd_j1_rot), which the diagonal orientations then take on both axes."""
    names = dtcwt_layout(o_dim, ri_dim)
    return _DTCWTFwdJ1.apply(x, _dtcwt_taps1(h0o, h1o, h2o), True, bool(skip_hps), names, int(mode))


def dtcwt_fwd_j2(x, h0a, h0b, h1a, h1b, skip_hps=False, o_dim=2, ri_dim=-1, h2a=None, h2b=None):
    """A level >= 2 of the forward transform: x (N, C, H, W), multiples of 4 -> (ll (N, C, H/2, W/2), highs (.., H/4, W/4, ..)).
    ``h2a``, ``h2b``: the bandpass pair of a three-filter bank (fwd_j2plus_rot)."""
    names = dtcwt_layout(o_dim, ri_dim)
    return _DTCWTFwdJ2.apply(x, _dtcwt_taps2(h0a, h0b, h1a, h1b, h2a, h2b), False, bool(skip_hps), names, 1)


def dtcwt_inv_j1(ll, highs, g0o, g1o, o_dim=2, ri_dim=-1, mode=1, g2o=None):
    """Level 1 of the inverse: ll (N, C, H, W) and highs (.., H/2, W/2, ..) -> y (N, C, H, W); either may be None for zeros.
    ``g2o``: the bandpass filter of a three-filter bank (inv_j1_rot)."""
    names = dtcwt_layout(o_dim, ri_dim)
    return _DTCWTInvJ1.apply(ll, highs, _dtcwt_taps1(g0o, g1o, g2o), True, names, int(mode))


def dtcwt_inv_j2(ll, highs, g0a, g0b, g1a, g1b, o_dim=2, ri_dim=-1, g2a=None, g2b=None):
    """A level >= 2 of the inverse: ll (N, C, R, Q) and highs (.., R/2, Q/2, ..) -> y (N, C, 2R, 2Q); either may be None.
    ``g2a``, ``g2b``: the bandpass pair of a three-filter bank (inv_j2plus_rot)."""
    names = dtcwt_layout(o_dim, ri_dim)
    return _DTCWTInvJ2.apply(ll, highs, _dtcwt_taps2(g0a, g0b, g1a, g1b, g2a, g2b), False, names, 1)


# ----------------------------------------------------------------------------------------
# DTCWT magnitude loss (csrc/dtcwt_loss.hip): both images' level in one launch, no band stored
# ----------------------------------------------------------------------------------------
DTCWT_LOSS_MAX_LEVELS = 16
_DTCWT_NAMES = ("n", "c", "o", "h", "w", "r")


def dtcwt_mag_loss_fused(H, W, J):
    """Whether an H x W image runs ``dtcwt_mag_loss`` on the fused kernels: both sides multiples of 2^J (no level pads)."""
    return 1 <= J <= DTCWT_LOSS_MAX_LEVELS and H >= (1 << J) and W >= (1 << J) and H % (1 << J) == 0 and W % (1 << J) == 0


def _dtcwt_mag_loss_check(x, y, taps2, J, mode, magbias, level_weights):
    """Every refusal of the magnitude loss, the device check last; returns the level weights as floats."""
    if int(J) != J or J < 1:
        raise ValueError("the magnitude loss takes J >= 1 levels, got %r" % (J,))
    if J >= 2 and taps2 is None:
        raise ValueError("J = %d needs the four q-shift filters (levels >= 2), got None" % J)
    if not magbias > 0:
        raise ValueError("magbias must be positive (the magnitude's gradient is z / r), got %r" % (magbias,))
    w = [1.0] * J if level_weights is None else [float(v) for v in level_weights]
    if len(w) != J:
        raise ValueError("level_weights lists one weight per level: %d entries for J = %d" % (len(w), J))
    if x.dim() != 4 or y.dim() != 4:
        raise ValueError("the magnitude loss takes inputs of 4 dimensions (N, C, H, W), got %d and %d" % (x.dim(), y.dim()))
    if x.shape != y.shape:
        raise ValueError("x and y must have the same shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError("the magnitude loss takes non-empty inputs, got %s" % (tuple(x.shape),))
    if not 0 <= mode <= 6:
        raise ValueError("Unkown pad type: {}".format(mode))
    for t, what in ((x, "x"), (y, "y")):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (what, t.dtype))
    _dtcwt_dev(x, "x")
    _dtcwt_dev(y, "y")
    if x.device != y.device:
        raise ValueError("x and y must be on one device, got %s and %s" % (x.device, y.device))
    return w


class _DTCWTMagLoss(Function):
    """``apply(x, y, taps1, taps2, J, mode, bias, weights, want_x, want_y) -> L`` on sizes ``dtcwt_mag_loss_fused`` accepts: J
    analysis launches that take both images and one that adds the partial sums.  The cotangent bands of an input that needs a
    gradient are written by the same launches (already scaled by w_j / count_j) and are all that is saved; the backward runs them
    through the transform's adjoint, coarsest level first -- J launches per input -- and scales by the upstream gradient on the
    device."""

    @staticmethod
    def forward(ctx, x, y, taps1, taps2, J, mode, bias, weights, want_x, want_y):
        N, C, H, W = x.shape
        dev = x.device
        lib = _lib.load()
        dims, floats = [], []
        h, w = H, W
        for j in range(J):
            n = lib.faoctasr_dtcwt_loss_workspace_floats(N, C, h, w, int(j == 0))
            if n < 0:
                raise _lib.KernelError("faoctasr_dtcwt_loss_workspace_floats failed: %s" % lib.faoctasr_last_error().decode())
            dims.append((h, w))
            floats.append(n)
            if j:
                h, w = h // 2, w // 2
        ws = _lib.workspace(dev, sum(floats), "dtcwt_loss")   # per stream: consumed by the same call's last launch
        out = torch.empty((), dtype=torch.float32, device=dev)
        scales, gxs, gys = [], [], []
        b2 = float(bias) * float(bias)
        off = 0
        for j in range(J):
            h, w = dims[j]
            bh, bw = (h // 2, w // 2) if j == 0 else (h // 4, w // 4)
            scales.append(weights[j] / float(N * C * 6 * bh * bw))
            last = j == J - 1
            lh, lw = (h, w) if j == 0 else (h // 2, w // 2)
            llx = None if last else torch.empty((N, C, lh, lw), dtype=torch.float32, device=dev)
            lly = None if last else torch.empty((N, C, lh, lw), dtype=torch.float32, device=dev)
            gx = torch.empty((N, C, 6, bh, bw, 2), dtype=torch.float32, device=dev) if want_x else None
            gy = torch.empty((N, C, 6, bh, bw, 2), dtype=torch.float32, device=dev) if want_y else None
            x, xn, xc, xr = _dtcwt_low(x)
            y, yn, yc, yr = _dtcwt_low(y)
            head = (x.data_ptr(), xn, xc, xr, y.data_ptr(), yn, yc, yr, ptr(llx), ptr(lly), ptr(gx), ptr(gy),
                    ws.data_ptr() + 4 * off, scales[j], b2, N, C, h, w)
            if j == 0:
                call("dtcwt_loss_fwd_j1", *head, _tap_array(taps1[0]), len(taps1[0]), _tap_array(taps1[1]), len(taps1[1]), mode, stream_ptr())
            else:
                call("dtcwt_loss_fwd_j2", *head, *(_tap_array(t) for t in taps2), len(taps2[0]), stream_ptr())
            off += floats[j]
            gxs.append(gx)
            gys.append(gy)
            x, y = llx, lly
        call("dtcwt_loss_final", ws.data_ptr(), ctypes.cast((ctypes.c_long * J)(*floats), ctypes.c_void_p),
             ctypes.cast((ctypes.c_double * J)(*scales), ctypes.c_void_p), J, ptr(out), stream_ptr())
        ctx.cfg = (taps1, _swap_ab(taps2) if taps2 is not None else None, mode, want_x, want_y)
        if want_x or want_y:
            ctx.save_for_backward(*[g for g in gxs + gys if g is not None])
        return out

    @staticmethod
    def backward(ctx, g):
        taps1, taps2, mode, want_x, want_y = ctx.cfg
        saved = list(ctx.saved_tensors)
        J = len(saved) // (int(want_x) + int(want_y)) if saved else 0
        grads = []
        for k, (want, need) in enumerate(((want_x, ctx.needs_input_grad[0]), (want_y, ctx.needs_input_grad[1]))):
            if not need:
                grads.append(None)
                continue
            if not want:
                raise _lib.KernelError("the magnitude loss's forward ran without gradients enabled for this input: no cotangent bands were saved")
            bands = saved[:J] if (k == 0 or not want_x) else saved[J:]
            low = None
            for h in bands[:0:-1]:
                low = _dtcwt_inverse(low, h, taps2, False, 1, _DTCWT_NAMES)
            grads.append(_dtcwt_inverse(low, bands[0], taps1, True, mode, _DTCWT_NAMES) * g)
        return tuple(grads) + (None,) * 8


def _dtcwt_mag_loss_composed(x, y, taps1, taps2, J, mode, bias, weights):
    """The same definition from the per-level ops, the modules' padding and torch ops: for sizes the fused kernels do not take."""
    b2 = float(bias) * float(bias)
    lows = []
    for t in (x, y):
        if t.shape[2] % 2:
            t = torch.cat((t, t[:, :, -1:]), dim=2)
        if t.shape[3] % 2:
            t = torch.cat((t, t[:, :, :, -1:]), dim=3)
        lows.append(t)
    total = None
    for j in range(J):
        mags = []
        for k in (0, 1):
            low = lows[k]
            if j == 0:
                low, h = _DTCWTFwdJ1.apply(low, taps1, True, False, _DTCWT_NAMES, mode)
            else:
                if low.shape[2] % 4:
                    low = torch.cat((low[:, :, 0:1], low, low[:, :, -1:]), dim=2)
                if low.shape[3] % 4:
                    low = torch.cat((low[:, :, :, 0:1], low, low[:, :, :, -1:]), dim=3)
                low, h = _DTCWTFwdJ2.apply(low, taps2, False, False, _DTCWT_NAMES, 1)
            lows[k] = low
            mags.append(torch.sqrt(h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + b2))
        term = weights[j] * (mags[0] - mags[1]).abs().mean()
        total = term if total is None else total + term
    return total


def dtcwt_mag_loss(x, y, h0o, h1o, qshift=None, J=1, mode=1, magbias=1e-2, level_weights=None):
    """``sum_j w_j * mean |r_j(x) - r_j(y)|`` with ``r = sqrt(re^2 + im^2 + magbias^2)`` over the six complex orientations of every
    level j = 1..J of the dual-tree transform of x and y (N, C, H, W), as a 0-d fp32 tensor with gradients to both; the mean of a
    level runs over its N * C * 6 * h_j * w_j coefficients, there is no lowpass term.  Filters as the modules register them (taps
    reversed): ``h0o``, ``h1o`` and, for J >= 2, ``qshift`` = (h0a, h0b, h1a, h1b).  ``mode`` acts on level 1: 1 is the symmetric
    extension, any other ``wavelets.mode_to_int`` code pads with zeros.  ``magbias`` > 0.

    With H and W multiples of 2^J the op is J + 1 launches of csrc/dtcwt_loss.hip -- a block runs its tile of x and then of y, and
    no band is stored -- and J launches of the transform's adjoint per input that needs a gradient; under ``no_grad`` nothing is
    saved.  Bit-reproducible.  Any other size takes the composition of the per-level ops with the modules' padding and torch ops
    for the magnitude and the mean: the same definition, autograd-correct, slower."""
    taps1 = _dtcwt_taps1(h0o, h1o)
    taps2 = _dtcwt_taps2(*qshift) if qshift is not None else None
    w = _dtcwt_mag_loss_check(x, y, taps2, J, int(mode), magbias, level_weights)
    J = int(J)
    if not dtcwt_mag_loss_fused(x.shape[2], x.shape[3], J):
        return _dtcwt_mag_loss_composed(x, y, taps1, taps2, J, int(mode), float(magbias), w)
    grad = torch.is_grad_enabled()
    return _DTCWTMagLoss.apply(x, y, taps1, taps2, J, int(mode), float(magbias), tuple(w), grad and x.requires_grad, grad and y.requires_grad)


# ----------------------------------------------------------------------------------------
# complex-wavelet structural similarity (csrc/cwssim.hip): a windowed complex correlation over the bands of a dual-tree level
# ----------------------------------------------------------------------------------------
CWSSIM_MAX_WIN = 11


def _cwssim_check_scalars(win, K):
    if int(win) != win or not 1 <= win <= CWSSIM_MAX_WIN:
        raise ValueError("the window side win must be an integer 1..%d, got %r" % (CWSSIM_MAX_WIN, win))
    if not (K > 0 and K < float("inf")):
        raise ValueError("the constant K must be positive and finite (it keeps the index defined where both bands vanish), got %r" % (K,))


def _cwssim_check_bands(hx, hy, win):
    """Every refusal of ``cw_ssim_bands`` that concerns the tensors, the device check last."""
    for t, what in ((hx, "hx"), (hy, "hy")):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (what, t.dtype))
        if t.dim() != 6 or t.shape[2] != 6 or t.shape[5] != 2:
            raise ValueError("%s must be a band tensor (N, C, 6, h, w, 2), got %s" % (what, tuple(t.shape)))
    if hx.shape != hy.shape:
        raise ValueError("hx and hy must have the same shape, got %s and %s" % (tuple(hx.shape), tuple(hy.shape)))
    if hx.shape[0] < 1 or hx.shape[1] < 1:
        raise ValueError("the index takes non-empty bands, got %s" % (tuple(hx.shape),))
    if hx.shape[3] < win or hx.shape[4] < win:
        raise ValueError("a %d x %d band holds no %d x %d window" % (hx.shape[3], hx.shape[4], win, win))
    for t, what in ((hx, "hx"), (hy, "hy")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if hx.device != hy.device:
        raise ValueError("hx and hy must be on one device, got %s and %s" % (hx.device, hy.device))


class _CWSSIMBands(Function):
    """``apply(hx, hy, win, K, per_image, want_x, want_y) -> S``: ``cwssim_index`` and ``cwssim_final`` forward; where an input needs
    a gradient the index launch also stores the two maps, which with the bands are all that is saved, and the backward is one
    ``cwssim_grad`` launch that writes the cotangents asked for and reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, hx, hy, win, K, per_image, want_x, want_y):
        N, C, _, h, w, _ = hx.shape
        dev = hx.device
        planes = N * C * 6
        n = _lib.load().faoctasr_cwssim_workspace_floats(planes, h, w, win)
        if n < 0:
            raise _lib.KernelError("faoctasr_cwssim_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "cwssim")                 # per stream: consumed by the same call's second launch
        map_a = map_b = None
        if want_x or want_y:
            map_a = torch.empty((planes, h - win + 1, w - win + 1, 2), dtype=torch.float32, device=dev)
            map_b = torch.empty((planes, h - win + 1, w - win + 1), dtype=torch.float32, device=dev)
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = torch.empty((), dtype=torch.float32, device=dev)
        call("cwssim_index", ptr(hx), ptr(hy), ptr(map_a), ptr(map_b), ws.data_ptr(), planes, h, w, win, K, stream_ptr())
        call("cwssim_final", ws.data_ptr(), N, planes, h, w, win, ptr(out_image), ptr(out_mean), stream_ptr())
        ctx.cfg = (win, per_image, want_x, want_y)
        if want_x or want_y:
            ctx.save_for_backward(hx, hy, map_a, map_b)
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        win, per_image, want_x, want_y = ctx.cfg
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return (None,) * 7
        if (need_x and not want_x) or (need_y and not want_y):
            raise _lib.KernelError("the index's forward ran without gradients enabled for this input: no maps were saved")
        hx, hy, map_a, map_b = ctx.saved_tensors
        N, C, _, h, w, _ = hx.shape
        gscale = g.contiguous() if per_image else (g / N).expand(N).contiguous()      # on the device: no host read
        gx = torch.empty_like(hx) if need_x else None
        gy = torch.empty_like(hy) if need_y else None
        call("cwssim_grad", ptr(hx), ptr(hy), ptr(map_a), ptr(map_b), ptr(gx), ptr(gy), ptr(gscale), N, N * C * 6, h, w, win, stream_ptr())
        return (gx, gy) + (None,) * 5


def cw_ssim_bands(hx, hy, win=7, K=0.01, per_image=False):
    """The complex-wavelet structural similarity of two bands ``(N, C, 6, h, w, 2)`` of one dual-tree level: the mean over n, c, the
    six orientations and the ``(h - win + 1) x (w - win + 1)`` valid positions p of a ``win x win`` box window of

        S_p = (2 |z_p| + K) / (E_p + K),   z_p = sum_W hx conj(hy),   E_p = sum_W |hx|^2 + sum_W |hy|^2,

    as a 0-d fp32 tensor, or per image as ``(N,)`` with ``per_image``; 0 < S <= 1, and a small translation of one image turns every
    coefficient of a window by nearly the same phase, which |z_p| does not see.  Gradients to both bands.  Two launches of
    csrc/cwssim.hip forward and one backward; under ``no_grad``, or for inputs that need no gradient, no map is stored.
    ``S(x, x) == 1`` with zero gradients and ``S(x, y) == S(y, x)`` hold bit for bit; runs are bit-reproducible.  Non-contiguous
    bands are copied.  No double backward."""
    _cwssim_check_scalars(win, K)
    _cwssim_check_bands(hx, hy, int(win))
    grad = torch.is_grad_enabled()
    return _CWSSIMBands.apply(hx.contiguous(), hy.contiguous(), int(win), float(K), bool(per_image), grad and hx.requires_grad,
                              grad and hy.requires_grad)


def _cwssim_check(x, y, taps1, taps2, J, mode, win, K, level_weights):
    """Every refusal of ``cw_ssim``, the device check last; returns the level weights as floats."""
    if int(J) != J or J < 1:
        raise ValueError("the index takes J >= 1 levels, got %r" % (J,))
    if J >= 2 and taps2 is None:
        raise ValueError("J = %d needs the q-shift filters (levels >= 2), got None" % J)
    if taps2 is not None and (len(taps1) == 3) != (len(taps2) == 6):
        raise ValueError("a three-filter level-1 bank (h2o) goes with the q-shift bandpass pair (h2ab) and a two-filter one without")
    _cwssim_check_scalars(win, K)
    w = [1.0] * J if level_weights is None else [float(v) for v in level_weights]
    if len(w) != J:
        raise ValueError("level_weights lists one weight per level: %d entries for J = %d" % (len(w), J))
    if not sum(w) > 0:
        raise ValueError("level_weights must have a positive sum (the index is their weighted mean), got %r" % (w,))
    if x.dim() != 4 or y.dim() != 4:
        raise ValueError("the index takes inputs of 4 dimensions (N, C, H, W), got %d and %d" % (x.dim(), y.dim()))
    if x.shape != y.shape:
        raise ValueError("x and y must have the same shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if min(x.shape) < 1:
        raise ValueError("the index takes non-empty inputs, got %s" % (tuple(x.shape),))
    if not 0 <= mode <= 6:
        raise ValueError("Unkown pad type: {}".format(mode))
    for t, what in ((x, "x"), (y, "y")):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (what, t.dtype))
    for j, (_, _, (bh, bw)) in enumerate(dtcwt_sizes(x.shape[2], x.shape[3], int(J))):
        if bh < win or bw < win:
            raise ValueError("level %d of a %d x %d image has bands of %d x %d, which hold no %d x %d window"
                             % (j + 1, x.shape[2], x.shape[3], bh, bw, win, win))
    _dtcwt_dev(x, "x")
    _dtcwt_dev(y, "y")
    if x.device != y.device:
        raise ValueError("x and y must be on one device, got %s and %s" % (x.device, y.device))
    return w


def cw_ssim(x, y, h0o, h1o, qshift=None, J=1, mode=1, win=7, K=0.01, level_weights=None, per_image=False, h2o=None, h2ab=None):
    """The complex-wavelet structural similarity of two images (N, C, H, W): ``S = sum_j w_j S_j / sum_j w_j`` with ``S_j`` the
    index ``cw_ssim_bands`` of the bands of level j = 1..J of the dual-tree transform of x and y; a 0-d fp32 tensor, or ``(N,)``
    with ``per_image``, with gradients to both images (the loss is ``1 - S``).  Filters as the modules register them (taps
    reversed): ``h0o``, ``h1o`` and, for J >= 2, ``qshift`` = (h0a, h0b, h1a, h1b); ``h2o`` and ``h2ab`` = (h2a, h2b) are the bandpass
    filters of a three-filter bank.  ``mode`` acts on level 1: 1 is the symmetric extension, any other ``wavelets.mode_to_int`` code
    pads with zeros.  ``level_weights``: one weight per level (default all 1), of positive sum.  Every level's bands must hold a
    window.

    The levels are the autograd ops of the transform with ``DTCWTForward``'s padding (an odd side repeats its last row / column, a
    lowpass side that is no multiple of 4 its first and last), so any size the transform takes runs: per level one analysis launch
    per image, ``cwssim_index`` and ``cwssim_final``; backward one ``cwssim_grad`` and the transform's adjoint."""
    taps1 = _dtcwt_taps1(h0o, h1o, h2o)
    taps2 = _dtcwt_taps2(*(tuple(qshift) + (tuple(h2ab) if h2ab is not None else ()))) if qshift is not None else None
    w = _cwssim_check(x, y, taps1, taps2, J, int(mode), win, K, level_weights)
    J, win = int(J), int(win)
    lows = []
    for t in (x, y):
        if t.shape[2] % 2:
            t = torch.cat((t, t[:, :, -1:]), dim=2)
        if t.shape[3] % 2:
            t = torch.cat((t, t[:, :, :, -1:]), dim=3)
        lows.append(t)
    total = None
    for j in range(J):
        bands = []
        for k in (0, 1):
            low = lows[k]
            if j == 0:
                low, h = _DTCWTFwdJ1.apply(low, taps1, True, False, _DTCWT_NAMES, int(mode))
            else:
                if low.shape[2] % 4:
                    low = torch.cat((low[:, :, 0:1], low, low[:, :, -1:]), dim=2)
                if low.shape[3] % 4:
                    low = torch.cat((low[:, :, :, 0:1], low, low[:, :, :, -1:]), dim=3)
                low, h = _DTCWTFwdJ2.apply(low, taps2, False, False, _DTCWT_NAMES, 1)
            lows[k] = low
            bands.append(h)
        term = w[j] * cw_ssim_bands(bands[0], bands[1], win, K, per_image)
        total = term if total is None else total + term
    return total / sum(w)


# ----------------------------------------------------------------------------------------
# DTCWT scattering layers (csrc/scat.hip): a dual-tree level, smoothed magnitudes and the pooled lowpass in one launch
# ----------------------------------------------------------------------------------------
def scat_sizes(H, W, order):
    """((padded input rows, cols), (output rows, cols)) of ``ScatLayer`` (order 1: even sides, a half) and ``ScatLayerj2`` (order 2:
    multiples of 8, a quarter)."""
    q = 2 if order == 1 else 8
    h, w = H + (-H) % q, W + (-W) % q
    return (h, w), ((h // 2, w // 2) if order == 1 else (h // 4, w // 4))


def _scat_check(x, taps2, mode, combine_colour):
    """Every refusal of a scattering layer, the device check last; returns (N, C, H, W)."""
    if x.dim() != 4:
        raise ValueError("a scattering layer takes inputs of 4 dimensions (N, C, H, W), got %d" % x.dim())
    N, C, H, W = x.shape
    if N < 1 or C < 1:
        raise ValueError("a scattering layer takes at least one image and one channel, got N %d C %d" % (N, C))
    if combine_colour and C != 3:
        raise ValueError("combine_colour takes 3 channels, got %d" % C)
    q = 2 if taps2 is None else 8
    if H % q or W % q or H < q or W < q:
        raise ValueError("the input of a %s-order scattering layer must have rows and columns that are a multiple of %d, got %d x %d"
                         % ("first" if taps2 is None else "second", q, H, W))
    if not 0 <= mode <= 6:
        raise ValueError("Unkown pad type: {}".format(mode))
    if taps2 is not None and mode != 1:
        raise NotImplementedError("the q-shift level of ScatLayerj2 extends symmetrically only (mode 1), got mode %d" % mode)
    _dtcwt_dev(x, "the input")
    return N, C, H, W


def _scat_low(t):
    """(pointer, n stride, c stride) of an (N, C, h, w) view with contiguous rows."""
    if t.shape[3] > 1 and t.stride(3) != 1 or t.shape[2] > 1 and t.stride(2) != t.shape[3]:
        raise _lib.KernelError("a scattering lowpass operand must have contiguous rows, got strides %s" % (t.stride(),))
    return t.data_ptr(), t.stride(0), t.stride(1)


def _scat_mag(t, colour):
    """(pointer, n, orientation and c strides) of an (N, 6, C, h, w) view with contiguous rows; the colour form has no c axis."""
    if t.shape[4] > 1 and t.stride(4) != 1 or t.shape[3] > 1 and t.stride(3) != t.shape[4] or t.shape[1] != 6:
        raise _lib.KernelError("a scattering magnitude operand must have 6 orientations and contiguous rows, got %s strides %s"
                               % (tuple(t.shape), t.stride()))
    return t.data_ptr(), t.stride(0), t.stride(1), (0 if colour else t.stride(2))


def _scat_fwd(x, taps, level1, mode, bias, low, pool, mag, phase, colour):
    """One forward launch: x (N, C, H, W) -> the views ``low`` (N, C, ., .), ``mag`` (N, 6, C or 1, ., .) and ``phase`` (or None)."""
    N, C, H, W = x.shape
    x, sn, sc, sr = _dtcwt_low(x)
    b = float(bias)
    if level1:
        call("scat_fwd_j1", x.data_ptr(), sn, sc, sr, *_scat_low(low), int(pool), *_scat_mag(mag, colour), ptr(phase),
             int(colour), b, b * b, N, C, H, W, *_taps1_args(taps), mode, stream_ptr())
    else:
        call("scat_fwd_j2", x.data_ptr(), sn, sc, sr, *_scat_low(low), *_scat_mag(mag, colour), ptr(phase), int(colour), b,
             b * b, N, C, H, W, *_taps2_args(taps), stream_ptr())


def _scat_bwd(dlow, pool, dmag, phase, taps, level1, mode, colour, shape):
    """One backward launch on the forward's taps: the cotangent views and the phasors -> dx of ``shape`` (N, C, H, W)."""
    N, C, H, W = shape
    dx = torch.empty(shape, dtype=torch.float32, device=phase.device)
    if level1:
        call("scat_bwd_j1", *_scat_low(dlow), int(pool), *_scat_mag(dmag, colour), ptr(phase), ptr(dx), N, C, H, W,
             *_taps1_args(taps), mode, stream_ptr())
    else:
        call("scat_bwd_j2", *_scat_low(dlow), *_scat_mag(dmag, colour), ptr(phase), ptr(dx), N, C, H, W, *_taps2_args(taps), stream_ptr())
    return dx


def _scat_phase(x, C, h, w, save):
    return torch.empty((x.shape[0], 6, C, h, w, 2), dtype=torch.float32, device=x.device) if save else None


class _ScatJ1(Function):
    """scatternet/lowlevel.py:71-137 ScatLayerj1_f on csrc/scat.hip: ``apply(x, taps, mode, bias, colour, save) -> Z`` of shape
    (N, 7, C, H/2, W/2), or (N, 9, H/2, W/2) with ``colour``; one launch, and one for the backward.  ``save`` False stores no
    phasors (the reference's ``x.requires_grad == False`` branch)."""

    @staticmethod
    def forward(ctx, x, taps, mode, bias, colour, save):
        N, C, H, W = x.shape
        h, w = H // 2, W // 2
        phase = _scat_phase(x, C, h, w, save)
        if colour:
            Z = torch.empty((N, 9, h, w), dtype=torch.float32, device=x.device)
            low, mag = Z[:, :3], Z[:, 3:].unsqueeze(2)
        else:
            Z = torch.empty((N, 7, C, h, w), dtype=torch.float32, device=x.device)
            low, mag = Z[:, 0], Z[:, 1:]
        _scat_fwd(x, taps, True, mode, bias, low, True, mag, phase, colour)
        ctx.cfg = (taps, mode, colour, tuple(x.shape))
        if save:
            ctx.save_for_backward(phase)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        taps, mode, colour, shape = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        if not ctx.saved_tensors:
            raise _lib.KernelError("the scattering layer's forward ran without gradients enabled: no phasors were saved")
        phase, = ctx.saved_tensors
        dZ = dZ.contiguous()
        dlow, dmag = (dZ[:, :3], dZ[:, 3:].unsqueeze(2)) if colour else (dZ[:, 0], dZ[:, 1:])
        return (_scat_bwd(dlow, True, dmag, phase, taps, True, mode, colour, shape),) + (None,) * 5


class _ScatJ2(Function):
    """scatternet/lowlevel.py:206-398 ScatLayerj2_f: ``apply(x, taps1, taps2, mode, bias, colour, save) -> Z`` of shape
    (N, 49, C, H/4, W/4), or (N, 51, H/4, W/4) with ``colour``.  Three launches write Z in place -- level 1 on x (unpooled lowpass
    s0 and first-order magnitudes, two temporaries), level 2 on s0, level 1 on the 6C (colour: 6) magnitude channels -- and the
    backward is the three adjoints in reverse."""

    @staticmethod
    def forward(ctx, x, taps1, taps2, mode, bias, colour, save):
        N, C, H, W = x.shape
        h2, w2, h4, w4 = H // 2, W // 2, H // 4, W // 4
        dev = x.device
        C1 = 1 if colour else C                                        # channels of a first-order magnitude
        s0 = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
        m1 = torch.empty((N, 6, C1, h2, w2), dtype=torch.float32, device=dev)
        ph1, ph2, ph21 = _scat_phase(x, C, h2, w2, save), _scat_phase(x, C, h4, w4, save), _scat_phase(x, 6 * C1, h4, w4, save)
        if colour:
            Z = torch.empty((N, 51, h4, w4), dtype=torch.float32, device=dev)
            z_s0, z_s1j1, z_s1j2, z_s2 = Z[:, :3], Z[:, 3:9], Z[:, 9:15].unsqueeze(2), Z[:, 15:].view(N, 6, 6, h4, w4)
        else:
            Z = torch.empty((N, 49, C, h4, w4), dtype=torch.float32, device=dev)
            z_s0, z_s1j1, z_s1j2, z_s2 = Z[:, 0], Z[:, 1:7].view(N, 6 * C, h4, w4), Z[:, 7:13], Z[:, 13:].view(N, 6, 6 * C, h4, w4)
        _scat_fwd(x, taps1, True, mode, bias, s0, False, m1, ph1, colour)
        _scat_fwd(s0, taps2, False, 1, bias, z_s0, True, z_s1j2, ph2, colour)
        _scat_fwd(m1.view(N, 6 * C1, h2, w2), taps1, True, mode, bias, z_s1j1, True, z_s2, ph21, False)
        ctx.cfg = (taps1, taps2, mode, colour, tuple(x.shape))
        if save:
            ctx.save_for_backward(ph1, ph2, ph21)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        taps1, taps2, mode, colour, shape = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        if not ctx.saved_tensors:
            raise _lib.KernelError("the scattering layer's forward ran without gradients enabled: no phasors were saved")
        ph1, ph2, ph21 = ctx.saved_tensors
        N, C, H, W = shape
        h2, w2, h4, w4 = H // 2, W // 2, H // 4, W // 4
        C1 = 1 if colour else C
        dZ = dZ.contiguous()
        if colour:
            d_s0, d_s1j1, d_s1j2, d_s2 = dZ[:, :3], dZ[:, 3:9], dZ[:, 9:15].unsqueeze(2), dZ[:, 15:].view(N, 6, 6, h4, w4)
        else:
            d_s0, d_s1j1, d_s1j2, d_s2 = dZ[:, 0], dZ[:, 1:7].view(N, 6 * C, h4, w4), dZ[:, 7:13], dZ[:, 13:].view(N, 6, 6 * C, h4, w4)
        dm1 = _scat_bwd(d_s1j1, True, d_s2, ph21, taps1, True, mode, False, (N, 6 * C1, h2, w2))
        ds0 = _scat_bwd(d_s0, True, d_s1j2, ph2, taps2, False, 1, colour, (N, C, H, W))
        dx = _scat_bwd(ds0, False, dm1.view(N, 6, C1, h2, w2), ph1, taps1, True, mode, colour, (N, C, H, W))
        return (dx,) + (None,) * 6


def scat_layer_j1(x, h0o, h1o, mode=1, magbias=1e-2, combine_colour=False, h2o=None):
    """One order of scattering at one scale: x (N, C, H, W), H and W even -> Z (N, 7, C, H/2, W/2): the 2x2 mean of the level-1
    lowpass, then ``sqrt(re^2 + im^2 + magbias^2) - magbias`` of the six orientations; with ``combine_colour`` (C == 3) the
    magnitude runs over the three channels too and Z is (N, 9, H/2, W/2).  Filters as the modules register them (taps reversed);
    ``mode`` 1 is the symmetric extension, any other ``wavelets.mode_to_int`` code pads with zeros.  ``h2o``: the bandpass filter
    of a three-filter bank (ScatLayerj1_rot_f)."""
    taps = _dtcwt_taps1(h0o, h1o, h2o)
    _scat_check(x, None, int(mode), combine_colour)
    return _ScatJ1.apply(x, taps, int(mode), float(magbias), bool(combine_colour), torch.is_grad_enabled() and x.requires_grad)


def scat_layer_j2(x, h0o, h1o, h0a, h0b, h1a, h1b, mode=1, magbias=1e-2, combine_colour=False, h2o=None, h2a=None, h2b=None):
    """Second-order scattering over two scales: x (N, C, H, W), multiples of 8 -> Z (N, 49, C, H/4, W/4): the lowpass, the six
    first-order magnitudes of level 1 (pooled) and of level 2, and the 36 second-order ones (index 6 o2 + o1); with
    ``combine_colour`` (N, 51, H/4, W/4) = 3 + 6 + 6 + 36.  Only ``mode`` 1 (symmetric), as in the reference.  ``h2o``, ``h2a``,
    ``h2b``: the bandpass filters of a three-filter bank (ScatLayerj2_rot_f), all three or none."""
    third = [t is not None for t in (h2o, h2a, h2b)]
    if any(third) and not all(third):
        raise ValueError("a three-filter bank takes all of h2o, h2a and h2b; got only %s"
                         % ", ".join(n for n, g in zip(("h2o", "h2a", "h2b"), third) if g))
    taps1, taps2 = _dtcwt_taps1(h0o, h1o, h2o), _dtcwt_taps2(h0a, h0b, h1a, h1b, h2a, h2b)
    _scat_check(x, taps2, int(mode), combine_colour)
    return _ScatJ2.apply(x, taps1, taps2, int(mode), float(magbias), bool(combine_colour), torch.is_grad_enabled() and x.requires_grad)


class _HaarDFront(Function):
    @staticmethod
    def forward(ctx, x, mode):
        x = _c(x)
        N, C, H, W = x.shape
        if C != 1:
            raise _lib.KernelError("discriminator front end expects single-channel images")
        y = torch.empty((N, 3 if mode else 1, H // 2, W // 2), dtype=torch.float32, device=x.device)
        call("haar_dfront_fwd", ptr(x), ptr(y), N, H, W, mode, stream_ptr())
        ctx.cfg = (N, H, W, mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, mode = ctx.cfg
        dy = _c(dy)
        dx = torch.empty((N, 1, H, W), dtype=torch.float32, device=dy.device)
        call("haar_dfront_bwd", ptr(dy), ptr(dx), N, H, W, mode, stream_ptr())
        return dx, None


def haar_dfront(x, mode):
    """mode 0: LL (FS_DiscriminatorA, model.py:171-172); 1: cat(LH,HL,HH)*0.5+0.5 (FS_DiscriminatorB, model.py:225-233)."""
    return _HaarDFront.apply(x, int(mode))


# ----------------------------------------------------------------------------------------
# FFT Gaussian split as circulant GEMMs
# ----------------------------------------------------------------------------------------
_circ_cache = {}


def circulant_lowpass(n, radius, device):
    """Real symmetric circulant C with C x == ifft(ifftshift(g) * fft(x)) for the centred Gaussian taps
    g[k] = exp(-(k - int(n/2))^2 / (2 r^2)) of utils.py:71-80 (the 2-D mask is the outer product g g^T).  Built on the device
    by ``faoctasr_circulant_lowpass`` once per (n, radius, device); this dict is the caller-owned filter cache of SURVEY 8b."""
    device = torch.device(device)
    key = (n, float(radius), device.type, device.index if device.index is not None else torch.cuda.current_device())
    c = _circ_cache.get(key)
    if c is None:
        if device.type != "cuda":
            raise _lib.KernelError("circulant_lowpass: the filter matrices are built by a HIP kernel; got device %s" % device)
        c = torch.empty((n, n), dtype=torch.float32, device=device)
        call("circulant_lowpass", ptr(c), n, float(radius), stream_ptr())
        _circ_cache[key] = c
    return c


def _lowpass2d(x3, ch, cw, st):
    """x3: (B,H,W) -> Ch @ x_b @ Cw for every b (two MFMA SGEMM launches)."""
    B, H, W = x3.shape
    t = torch.empty_like(x3)
    call("sgemm_batched", ptr(x3), ptr(cw), ptr(t), B * H, W, W, W, W, W, 0, 0, 0, 1, st)
    y = torch.empty_like(x3)
    call("sgemm_batched", ptr(ch), ptr(t), ptr(y), H, W, H, H, W, W, 0, H * W, H * W, B, st)
    return y


class _FreqSplit(Function):
    @staticmethod
    def forward(ctx, x, r_hp, r_lp):
        x = _c(x)
        B, C, H, W = x.shape
        dev = x.device
        mats = (circulant_lowpass(H, r_hp, dev), circulant_lowpass(W, r_hp, dev), circulant_lowpass(H, r_lp, dev), circulant_lowpass(W, r_lp, dev))
        st = stream_ptr()
        x3 = x.view(B * C, H, W)
        low_hp = _lowpass2d(x3, mats[0], mats[1], st)
        low_lp = _lowpass2d(x3, mats[2], mats[3], st)
        hf, lf = torch.empty_like(x), torch.empty_like(x)
        call("freq_mix_fwd", ptr(x), ptr(low_hp), ptr(low_lp), ptr(hf), ptr(lf), x.numel(), st)
        ctx.save_for_backward(x, low_hp, low_lp)
        ctx.mats = mats
        return hf, lf

    @staticmethod
    def backward(ctx, g_hf, g_lf):
        x, low_hp, low_lp = ctx.saved_tensors
        mats = ctx.mats
        st = stream_ptr()
        B, C, H, W = x.shape
        s_hp, s_lp, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        call("freq_mix_bwd", ptr(x), ptr(low_hp), ptr(low_lp), ptr(_c(g_hf)) if g_hf is not None else None,
             ptr(_c(g_lf)) if g_lf is not None else None, ptr(s_hp), ptr(s_lp), ptr(dx), x.numel(), st)
        # the circulants are symmetric (to the bit: circulant_lowpass_kernel), so the adjoint of x -> Ch x Cw is the same map
        a = _lowpass2d(s_hp.view(B * C, H, W), mats[0], mats[1], st)
        b = _lowpass2d(s_lp.view(B * C, H, W), mats[2], mats[3], st)
        n = x.numel()
        call("axpby", ptr(dx), ptr(a), ptr(dx), n, 1.0, -1.0, st)
        call("axpby", ptr(dx), ptr(b), ptr(dx), n, 1.0, 1.0, st)
        return dx, None, None


def freq_split(x, r_hp, r_lp):
    """hf = (high_pass(x_b, r_hp) + x_b)/2, lf = low_pass(x_b, r_lp) per sample (train.py:173-175)."""
    return _FreqSplit.apply(x, float(r_hp), float(r_lp))


# ----------------------------------------------------------------------------------------
# spectral phase-consistency loss (model.py:36-58) as DFT GEMMs
# ----------------------------------------------------------------------------------------
_dft_cache = {}


def dft_tables(n, device):
    """The cos / sin tables of the n-point DFT, ``[C_n | S_n]`` followed by ``[C_n ; S_n]`` (4 n^2 floats), built on the device by
    ``faoctasr_dft_tables`` once per (n, device) on the calling stream; cached here next to the circulants.  A caller that uses
    the tables from several streams builds them before it forks (``TrainStep.step`` does)."""
    device = torch.device(device)
    key = (n, device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _dft_cache.get(key)
    if t is None:
        if device.type != "cuda":
            raise _lib.KernelError("dft_tables: the tables are built by a HIP kernel; got device %s" % device)
        t = torch.empty(4 * n * n, dtype=torch.float32, device=device)
        call("dft_tables", ptr(t), n, stream_ptr())
        _dft_cache[key] = t
    return t


class _PhaseLoss(Function):
    @staticmethod
    def forward(ctx, x, y, radius):
        x, y = _c(x), _c(y)
        if x.dim() != 4 or x.shape != y.shape:
            raise _lib.KernelError("phase_loss operands must be (B,C,H,W) tensors of one shape: %s vs %s" % (tuple(x.shape), tuple(y.shape)))
        N, C, H, W = x.shape
        tab_h, tab_w = dft_tables(H, x.device), dft_tables(W, x.device)
        n = _lib.load().faoctasr_phase_loss_workspace_floats(N, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_phase_loss_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        # the workspace carries the spectrum planes to the backward, so it belongs to this call (not to the per-stream scratch)
        ws = torch.empty(n, dtype=torch.float32, device=x.device)
        per_sample = torch.empty(N, dtype=torch.float32, device=x.device)
        mean = torch.empty((), dtype=torch.float32, device=x.device)
        call("phase_loss_fwd", ptr(x), ptr(y), ptr(tab_h), ptr(tab_w), radius, ptr(per_sample), ptr(mean), ptr(ws), N, C, H, W, stream_ptr())
        ctx.save_for_backward(ws, tab_h, tab_w)
        ctx.cfg = (radius, N, C, H, W)
        return mean

    @staticmethod
    def backward(ctx, g):
        ws, tab_h, tab_w = ctx.saved_tensors
        radius, N, C, H, W = ctx.cfg
        g = _c(g)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[0] else None
        dy = torch.empty((N, C, H, W), dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[1] else None
        call("phase_loss_bwd", ptr(g), ptr(tab_h), ptr(tab_w), radius, ptr(dx), ptr(dy), ptr(ws), N, C, H, W, stream_ptr())
        return dx, dy, None


def phase_loss(x, y, radius=5.0):
    """``phase_consistency_loss()(x, y)`` of model.py:36-58: minus the cosine similarity of the mask-weighted log-amplitude
    spectra of ``x`` and ``y`` (B,C,H,W), as a 0-dim tensor with gradients to both inputs.  The reference reads sample 0 only
    (its train.py runs batch 1); here the loss is evaluated per sample and averaged over the batch, which is the same thing at
    B = 1 (the rule of ``high_pass`` / ``low_pass``).  A spectrum bin of exactly zero amplitude gives NaN, as in the reference.
    Always exact fp32 (``conv_precision`` does not apply)."""
    return _PhaseLoss.apply(x, y, float(radius))


# ----------------------------------------------------------------------------------------
# focal frequency loss (Jiang et al., ICCV 2021) on the same DFT GEMMs
# ----------------------------------------------------------------------------------------
def check_ffl_alpha(alpha):
    """``alpha`` of the focal frequency loss as a float; finite and >= 0, or ValueError."""
    alpha = float(alpha)
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError("focal frequency loss: alpha must be finite and >= 0, got %r" % alpha)
    return alpha


class _FocalFrequencyLoss(Function):
    @staticmethod
    def forward(ctx, x, y, alpha, log_matrix, batch_matrix, save):
        x, y = _c(x), _c(y)
        N, C, H, W = x.shape
        tab_h, tab_w = dft_tables(H, x.device), dft_tables(W, x.device)
        n = _lib.load().faoctasr_ffl_workspace_floats(N, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_ffl_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = torch.empty(n, dtype=torch.float32, device=x.device)        # scratch of this call: free again behind it on the stream
        out = torch.empty((), dtype=torch.float32, device=x.device)
        # Re, -Im of the difference spectrum and 1 / phi(M) per plane: stored only when a backward can follow (``save``)
        planes = torch.empty(N * C * (2 * H * W + 1), dtype=torch.float32, device=x.device) if save else None
        call("ffl_fwd", ptr(x), ptr(y), ptr(tab_h), ptr(tab_w), alpha, int(log_matrix), int(batch_matrix), ptr(out), ptr(planes), ptr(ws),
             N, C, H, W, stream_ptr())
        if save:
            ctx.save_for_backward(planes, tab_h, tab_w)
        ctx.cfg = (alpha, int(log_matrix), N, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        planes, tab_h, tab_w = ctx.saved_tensors
        alpha, log_matrix, N, C, H, W = ctx.cfg
        g = _c(g)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=planes.device) if ctx.needs_input_grad[0] else None
        dy = torch.empty((N, C, H, W), dtype=torch.float32, device=planes.device) if ctx.needs_input_grad[1] else None
        ws = torch.empty(_lib.load().faoctasr_ffl_workspace_floats(N, C, H, W), dtype=torch.float32, device=planes.device)
        call("ffl_bwd", ptr(g), ptr(planes), ptr(tab_h), ptr(tab_w), alpha, log_matrix, ptr(dx), ptr(dy), ptr(ws), N, C, H, W, stream_ptr())
        return dx, dy, None, None, None, None


def focal_frequency_loss(x, y, alpha=1.0, log_matrix=False, batch_matrix=False):
    """The focal frequency loss of Jiang, Dai, Wu and Loy (ICCV 2021) for x, y (N,C,H,W) fp32 on one GPU, as a 0-dim fp32 tensor
    with gradients to both inputs: with ``D = fft2(x, norm="ortho") - fft2(y, norm="ortho")`` and ``q = |D|^2`` per plane,
    ``mean(w * q)`` where ``w = sqrt(q)^alpha`` (``log_matrix``: ``log(w + 1)``), divided by its maximum over the plane
    (``batch_matrix``: over the whole batch), NaN -> 0, and detached.  ``alpha = 0`` is the mean squared error.  One transform of
    ``x - y`` serves both images and the forward is one pass (csrc/spectral.hip); ``dL/dy`` is the exact negation of ``dL/dx``.
    The paper's ``patch_factor`` and ``ave_spectrum`` are not offered; no double backward.  Bit-reproducible, always exact fp32
    (``conv_precision`` does not apply)."""
    alpha = check_ffl_alpha(alpha)
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.dim() != 4 or x.shape != y.shape:
        raise _lib.KernelError("focal_frequency_loss operands must be (N,C,H,W) tensors of one shape: %s vs %s"
                               % (tuple(getattr(x, "shape", ())), tuple(getattr(y, "shape", ()))))
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise _lib.KernelError("focal_frequency_loss operands must be fp32, got %s and %s" % (x.dtype, y.dtype))
    if not (x.is_cuda and y.is_cuda) or x.device != y.device:
        raise _lib.KernelError("focal_frequency_loss runs as HIP kernels on one GPU; got devices %s and %s" % (x.device, y.device))
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise _lib.KernelError("focal_frequency_loss needs H, W >= 2, got %s" % (tuple(x.shape),))
    save = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)         # grad mode is off inside Function.forward
    return _FocalFrequencyLoss.apply(x, y, alpha, bool(log_matrix), bool(batch_matrix), save)


# ----------------------------------------------------------------------------------------
# spectral-profile loss (after Durall, Keuper, Keuper, CVPR 2020) on the half-spectrum DFT GEMMs
# ----------------------------------------------------------------------------------------
SPROF_MAX_SIDE = 1024
_radial_cache = {}
_sprof_geom_cache = {}
_sprof_half_cache = {}


def radial_bins(H, W):
    """``(bin, cnt)`` of the azimuthal average of an H x W spectrum, on the host: ``bin`` int64 (H, W), the ring of every UNSHIFTED
    frequency, ``floor(M sqrt(u_c^2/H^2 + v_c^2/W^2))`` with ``M = min(H, W)`` and centred ``u_c = ((u + H//2) mod H) - H//2``; ``cnt``
    int64 (K,), the positions per ring, ``K = 1 + floor(M sqrt((H//2)^2/H^2 + (W//2)^2/W^2))``.  Exact: the floor is settled in
    int64 (the largest k with ``k^2 H^2 W^2 <= M^2 (u_c^2 W^2 + v_c^2 H^2)``), a floating square root only proposes it.  No ring is
    empty and ``bin(u, v) == bin(-u, -v)``.  2 <= H, W <= 1024; cached, so do not write into the result."""
    if isinstance(H, bool) or isinstance(W, bool) or not (isinstance(H, int) and isinstance(W, int)) or not (2 <= H <= SPROF_MAX_SIDE and 2 <= W <= SPROF_MAX_SIDE):
        raise ValueError("radial_bins: H and W must be ints in [2, %d], got %r and %r" % (SPROF_MAX_SIDE, H, W))
    hit = _radial_cache.get((H, W))
    if hit is not None:
        return hit
    M = min(H, W)
    uc = ((torch.arange(H, dtype=torch.int64) + H // 2) % H - H // 2)[:, None]
    vc = ((torch.arange(W, dtype=torch.int64) + W // 2) % W - W // 2)[None, :]
    num, den = M * M * (uc * uc * (W * W) + vc * vc * (H * H)), H * H * W * W
    k = torch.sqrt(num.double() / den).floor().long()
    for _ in range(3):                                       # the proposal is off by at most one; three rounds leave a margin
        k = k + ((k + 1) * (k + 1) * den <= num).long() - (k * k * den > num).long()
    if not bool(((k * k * den <= num) & ((k + 1) * (k + 1) * den > num)).all()):
        raise AssertionError("radial_bins: the integer floor did not settle at %d x %d" % (H, W))
    K = 1 + math.isqrt(M * M * ((H // 2) ** 2 * W * W + (W // 2) ** 2 * H * H) // den)
    cnt = torch.bincount(k.flatten(), minlength=K)
    if cnt.numel() != K or int(cnt.min()) < 1 or int(cnt.sum()) != H * W:
        raise AssertionError("radial_bins: %d x %d gave %d bins for K = %d, smallest count %d" % (H, W, cnt.numel(), K, int(cnt.min())))
    _radial_cache[(H, W)] = (k, cnt)
    return k, cnt


def _dev_key(device):
    device = torch.device(device)
    return device, (device.type, device.index if device.index is not None else torch.cuda.current_device())


def sprof_half_tables(W, device, full=False):
    """The half-spectrum tables of the W-point DFT for the spectral profile, cut from ``dft_tables(W)`` once per (W, device):
    ``[C_W[:, :Wh] | S_W[:, :Wh]]`` (W x 2Wh) followed by its transpose stacked ``[C^T ; S^T]`` (2Wh x W), ``Wh = W//2 + 1``
    (``full``, a measuring switch: ``Wh = W``).  Like the DFT tables, built before any stream forks or a capture begins."""
    device, dk = _dev_key(device)
    key = (W, bool(full)) + dk
    t = _sprof_half_cache.get(key)
    if t is None:
        Wh = W if full else W // 2 + 1
        cs = dft_tables(W, device)[:2 * W * W].view(W, 2 * W)
        c, s = cs[:, :Wh], cs[:, W:W + Wh]
        t = torch.cat((torch.cat((c, s), 1).reshape(-1), torch.cat((c.t(), s.t()), 0).reshape(-1))).contiguous()
        _sprof_half_cache[key] = t
    return t


def sprof_host_geometry(H, W, full=False):
    """``(K, Wh, csr_off int32 (K+1,), csr_idx int32 (H*Wh,), cnt int32 (K,), binmap int16 (H, Wh))`` on the host, from
    ``radial_bins``: the half-plane positions (columns < ``Wh = W//2 + 1``; ``full``: every column) sorted by (bin, position) with
    their offsets per bin, the FULL-plane counts, and the bin of every half-plane position."""
    bins, cnt = radial_bins(H, W)
    K, Wh = cnt.numel(), (W if full else W // 2 + 1)
    half = bins[:, :Wh].contiguous()
    flat = half.flatten()
    off = torch.zeros(K + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(flat, minlength=K), 0)
    return K, Wh, off.int(), torch.argsort(flat, stable=True).int(), cnt.int(), half.short()


def sprof_geometry(H, W, device, full=False):
    """``sprof_host_geometry`` on the device, what the spectral-profile kernels read besides the DFT tables: built once per
    (H, W, device)."""
    device, dk = _dev_key(device)
    key = (H, W, bool(full)) + dk
    g = _sprof_geom_cache.get(key)
    if g is None:
        if device.type != "cuda":
            raise _lib.KernelError("spectral profile: the kernels run on a GPU; got device %s" % device)
        g = tuple(t.to(device) if torch.is_tensor(t) else t for t in sprof_host_geometry(H, W, full))
        _sprof_geom_cache[key] = g
    return g


def sprof_tables(H, W, device, full=False):
    """Every table of one (H, W, device): ``TrainStep.step`` calls this before its streams fork."""
    return (dft_tables(H, device), sprof_half_tables(W, device, full)) + sprof_geometry(H, W, device, full)


def check_sprof_params(eps, k_min):
    """``(eps, k_min)`` of the spectral-profile loss as a float and an int: eps finite and > 0, k_min an int >= 0, or ValueError
    (``k_min < K`` is checked against the shape)."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps > 0):
        raise ValueError("spectral profile loss: eps must be a finite number > 0, got %r" % (eps,))
    if isinstance(k_min, bool) or not isinstance(k_min, int) or k_min < 0:
        raise ValueError("spectral profile loss: k_min must be an int >= 0, got %r" % (k_min,))
    return float(eps), k_min


def _sprof_ws(sides, N, C, H, W, Wh, K, device):
    n = _lib.load().faoctasr_sprof_workspace_floats(sides, N, C, H, W, Wh, K)
    if n < 0:
        raise _lib.KernelError("faoctasr_sprof_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)         # scratch of this call: free again behind it on the stream


def _check_sprof_operands(what, *ts):
    for x in ts:
        if not torch.is_tensor(x) or x.dim() != 4:
            raise _lib.KernelError("%s operands must be (N,C,H,W) tensors, got %s" % (what, tuple(getattr(x, "shape", ()))))
    for x in ts:
        if x.dtype != torch.float32:
            raise _lib.KernelError("%s operands must be fp32, got %s" % (what, x.dtype))
    for x in ts:
        if not x.is_cuda:
            raise _lib.KernelError("%s runs as HIP kernels on one GPU; got device %s" % (what, x.device))
        if not (2 <= x.shape[2] <= SPROF_MAX_SIDE and 2 <= x.shape[3] <= SPROF_MAX_SIDE):
            raise _lib.KernelError("%s needs 2 <= H, W <= %d, got %s" % (what, SPROF_MAX_SIDE, tuple(x.shape)))


def sprof_loss_forward(x, y, eps=1e-8, k_min=1, batch_profile=False, per_image=False, save_x=False, save_y=False, full=False):
    """The forward launches of the spectral-profile loss without autograd: ``(loss 0-dim, per_image (N,) or None, profiles
    (2, N, C, K), saved_x, saved_y)``; ``saved_*`` (planes and coefficient table) only where ``save_*`` asks."""
    x, y = _c(x), _c(y)
    N, C, H, W = x.shape
    tab_h, half_w, K, Wh, off, idx, cnt, _ = sprof_tables(H, W, x.device, full)
    dev = x.device
    ws = _sprof_ws(2, N, C, H, W, Wh, K, dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    per = torch.empty(N, dtype=torch.float32, device=dev) if per_image else None
    prof = torch.empty((2, N, C, K), dtype=torch.float32, device=dev)
    sx = torch.empty(N * C * (2 * H * Wh + K), dtype=torch.float32, device=dev) if save_x else None
    sy = torch.empty(N * C * (2 * H * Wh + K), dtype=torch.float32, device=dev) if save_y else None
    call("sprof_loss_fwd", ptr(x), ptr(y), ptr(tab_h), ptr(half_w), off.data_ptr(), idx.data_ptr(), cnt.data_ptr(), eps, k_min,
         int(batch_profile), int(per_image), ptr(out), ptr(per), ptr(prof), ptr(sx), ptr(sy), ptr(ws), N, C, H, W, Wh, K, stream_ptr())
    return out, per, prof, sx, sy


class _SpectralProfileLoss(Function):
    @staticmethod
    def forward(ctx, x, y, eps, k_min, batch_profile, per_image, save_x, save_y, full):
        out, per, _, sx, sy = sprof_loss_forward(x, y, eps, k_min, batch_profile, per_image, save_x, save_y, full)
        ctx.save_for_backward(sx, sy)
        ctx.cfg = (per_image, full) + tuple(x.shape)
        ctx.dev = x.device
        return per if per_image else out

    @staticmethod
    def backward(ctx, g):
        sx, sy = ctx.saved_tensors
        per_image, full, N, C, H, W = ctx.cfg
        tab_h, half_w, K, Wh, _, _, cnt, binmap = sprof_tables(H, W, ctx.dev, full)
        g = _c(g)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=ctx.dev) if ctx.needs_input_grad[0] else None
        dy = torch.empty((N, C, H, W), dtype=torch.float32, device=ctx.dev) if ctx.needs_input_grad[1] else None
        ws = _sprof_ws(2, N, C, H, W, Wh, K, ctx.dev)
        call("sprof_bwd", ptr(g), int(per_image), None, ptr(sx), ptr(sy), ptr(tab_h), ptr(half_w), binmap.data_ptr(), cnt.data_ptr(), ptr(dx),
             ptr(dy), ptr(ws), N, C, H, W, Wh, K, stream_ptr())
        return (dx, dy) + (None,) * 7


def spectral_profile_loss(x, y, eps=1e-8, k_min=1, batch_profile=False, per_image=False, _full_spectrum=False):
    """The spectral-profile loss of x, y (N,C,H,W) fp32 on one GPU, 2 <= H, W <= 1024, with gradients to both inputs: with
    ``A[n,c,k]`` the azimuthally averaged power spectrum ``|fft2|^2 / (HW)`` over the rings of ``radial_bins(H, W)`` and ``a =
    log(A + eps)``, the mean over n, c and k >= ``k_min`` of ``(a_x - a_y)^2`` (0-dim; ``per_image``: (N,), each sample's mean over c
    and k).  ``batch_profile``: ``a`` is first averaged over n and c and the loss is the mean over k >= ``k_min`` of the squared
    difference of the two batch means -- phase-blind, translation-invariant and one short vector per domain, so x and y need not be
    paired (a fake against real images of the domain it should belong to).  ``k_min = 1`` drops the DC ring (the mean brightness).
    After Durall, Keuper and Keuper (CVPR 2020), whose binary cross-entropy on min-max-normalised profiles has no gradient at the
    extremes; this is the squared distance of log-profiles.  Only the half spectrum is transformed (csrc/spectral.hip).  Nothing is
    kept for a side that needs no gradient; no double backward.  Bit-reproducible, ``L(x, y) == L(y, x)`` bit for bit, always exact
    fp32 (``conv_precision`` does not apply)."""
    eps, k_min = check_sprof_params(eps, k_min)
    if per_image and batch_profile:
        raise ValueError("spectral profile loss: per_image has no meaning with batch_profile (one value per batch)")
    _check_sprof_operands("spectral_profile_loss", x, y)
    if x.shape != y.shape:
        raise _lib.KernelError("spectral_profile_loss operands must have one shape: %s vs %s" % (tuple(x.shape), tuple(y.shape)))
    if x.device != y.device:
        raise _lib.KernelError("spectral_profile_loss runs as HIP kernels on one GPU; got devices %s and %s" % (x.device, y.device))
    K = radial_bins(x.shape[2], x.shape[3])[1].numel()
    if k_min >= K:
        raise ValueError("spectral profile loss: k_min %d must be below the %d rings of a %d x %d spectrum" % (k_min, K, x.shape[2], x.shape[3]))
    grad = torch.is_grad_enabled()                                                   # grad mode is off inside Function.forward
    return _SpectralProfileLoss.apply(x, y, eps, k_min, bool(batch_profile), bool(per_image), grad and x.requires_grad, grad and y.requires_grad,
                                      bool(_full_spectrum))


class _SpectralProfile(Function):
    @staticmethod
    def forward(ctx, x, save, full):
        x = _c(x)
        N, C, H, W = x.shape
        tab_h, half_w, K, Wh, off, idx, cnt, _ = sprof_tables(H, W, x.device, full)
        ws = _sprof_ws(1, N, C, H, W, Wh, K, x.device)
        A = torch.empty((N, C, K), dtype=torch.float32, device=x.device)
        planes = torch.empty(N * C * 2 * H * Wh, dtype=torch.float32, device=x.device) if save else None
        call("sprof_profile_fwd", ptr(x), ptr(tab_h), ptr(half_w), off.data_ptr(), idx.data_ptr(), cnt.data_ptr(), ptr(A), ptr(planes), ptr(ws),
             N, C, H, W, Wh, K, stream_ptr())
        ctx.save_for_backward(planes)
        ctx.cfg = (full, N, C, H, W)
        return A

    @staticmethod
    def backward(ctx, gA):
        full, N, C, H, W = ctx.cfg
        planes, = ctx.saved_tensors
        tab_h, half_w, K, Wh, _, _, cnt, binmap = sprof_tables(H, W, planes.device, full)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=planes.device)
        ws = _sprof_ws(1, N, C, H, W, Wh, K, planes.device)
        call("sprof_bwd", None, 0, ptr(_c(gA)), ptr(planes), None, ptr(tab_h), ptr(half_w), binmap.data_ptr(), cnt.data_ptr(), ptr(dx), None,
             ptr(ws), N, C, H, W, Wh, K, stream_ptr())
        return dx, None, None


def spectral_profile(x, _full_spectrum=False):
    """The azimuthally averaged power spectrum of x (N,C,H,W) fp32 on one GPU, 2 <= H, W <= 1024: ``A[n,c,k]``, the mean of
    ``|fft2(x[n,c])|^2 / (HW)`` over ring k of ``radial_bins(H, W)``, (N, C, K) fp32, differentiable (no double backward).
    ``sum_k cnt_k A[k] = sum x^2`` (Parseval).  The launches of ``spectral_profile_loss`` for one image."""
    _check_sprof_operands("spectral_profile", x)
    return _SpectralProfile.apply(x, torch.is_grad_enabled() and x.requires_grad, bool(_full_spectrum))


# ----------------------------------------------------------------------------------------
# Fourier ring correlation (Saxton & Baumeister 1982; van Heel & Schatz 2005) on the spectral profile's half-spectrum path
# ----------------------------------------------------------------------------------------
FRC_MAX_SMOOTH = 15


def check_frc_params(k_min=1, k_max=None, eps=1e-16):
    """``(k_min, k_max, eps)`` of the Fourier ring correlation: k_min an int >= 0, k_max None or an int >= k_min, eps finite and > 0,
    or ValueError (``k_max <= K - 1`` is checked against the shape, ``frc_band``)."""
    if isinstance(k_min, bool) or not isinstance(k_min, int) or k_min < 0:
        raise ValueError("frc: k_min must be an int >= 0, got %r" % (k_min,))
    if k_max is not None and (isinstance(k_max, bool) or not isinstance(k_max, int) or k_max < k_min):
        raise ValueError("frc: k_max must be None or an int >= k_min = %d, got %r" % (k_min, k_max))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps > 0):
        raise ValueError("frc: eps must be a finite number > 0, got %r" % (eps,))
    return k_min, k_max, float(eps)


def frc_band(H, W, k_min=1, k_max=None):
    """``(k_min, k_max, K)`` for an H x W spectrum: ``k_max = None`` is the Nyquist ring ``min(H, W) // 2`` (the rings beyond it are
    the incomplete corner rings); ``0 <= k_min <= k_max <= K - 1`` or ValueError."""
    K = radial_bins(H, W)[1].numel()
    if k_max is None:
        k_max = min(H, W) // 2
    if not 0 <= k_min <= k_max <= K - 1:
        raise ValueError("frc: the band needs 0 <= k_min <= k_max <= %d (a %d x %d spectrum has %d rings), got k_min %r, k_max %r"
                         % (K - 1, H, W, K, k_min, k_max))
    return k_min, k_max, K


def _check_frc_operands(what, x, y):
    _check_sprof_operands(what, x, y)
    if x.shape != y.shape:
        raise _lib.KernelError("%s operands must have one shape: %s vs %s" % (what, tuple(x.shape), tuple(y.shape)))
    if x.device != y.device:
        raise _lib.KernelError("%s runs as HIP kernels on one GPU; got devices %s and %s" % (what, x.device, y.device))


def _frc_ws(N, C, H, W, Wh, K, device):
    n = _lib.load().faoctasr_frc_workspace_floats(N, C, H, W, Wh, K)
    if n < 0:
        raise _lib.KernelError("faoctasr_frc_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)         # scratch of this call: free again behind it on the stream


def frc_forward(x, y, k_min=1, k_max=None, eps=1e-16, per_image=False, save=False):
    """The forward launches of the Fourier ring correlation without autograd: ``(index 0-dim, per_image (N,) or None, curve
    (N, C, K), rings (3, N, C, K): the ring means Nk, Xk, Yk, saved)``; ``saved`` (both spectra and the coefficient tables) only where
    ``save`` asks.  ``rings[1]`` / ``rings[2]`` are ``spectral_profile(x)`` / ``(y)`` bit for bit."""
    x, y = _c(x), _c(y)
    N, C, H, W = x.shape
    k_min, k_max, _ = frc_band(H, W, k_min, k_max)
    tab_h, half_w, K, Wh, off, idx, cnt, _ = sprof_tables(H, W, x.device)
    dev = x.device
    ws = _frc_ws(N, C, H, W, Wh, K, dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    per = torch.empty(N, dtype=torch.float32, device=dev) if per_image else None
    curve = torch.empty((N, C, K), dtype=torch.float32, device=dev)
    rings = torch.empty((3, N, C, K), dtype=torch.float32, device=dev)
    saved = torch.empty(N * C * (4 * H * Wh + 3 * K), dtype=torch.float32, device=dev) if save else None
    call("frc_fwd", ptr(x), ptr(y), ptr(tab_h), ptr(half_w), off.data_ptr(), idx.data_ptr(), cnt.data_ptr(), eps, k_min, k_max,
         int(per_image), ptr(out), ptr(per), ptr(curve), ptr(rings), ptr(saved), ptr(ws), N, C, H, W, Wh, K, stream_ptr())
    return out, per, curve, rings, saved


class _FRC(Function):
    @staticmethod
    def forward(ctx, x, y, k_min, k_max, eps, per_image, save):
        out, per, _, _, saved = frc_forward(x, y, k_min, k_max, eps, per_image, save)
        ctx.save_for_backward(saved)
        ctx.cfg = (per_image,) + tuple(x.shape)
        ctx.dev = x.device
        return per if per_image else out

    @staticmethod
    def backward(ctx, g):
        saved, = ctx.saved_tensors
        per_image, N, C, H, W = ctx.cfg
        tab_h, half_w, K, Wh, _, _, _, binmap = sprof_tables(H, W, ctx.dev)
        g = _c(g)
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=ctx.dev) if ctx.needs_input_grad[0] else None
        dy = torch.empty((N, C, H, W), dtype=torch.float32, device=ctx.dev) if ctx.needs_input_grad[1] else None
        ws = _frc_ws(N, C, H, W, Wh, K, ctx.dev)
        call("frc_bwd", ptr(g), int(per_image), ptr(saved), ptr(tab_h), ptr(half_w), binmap.data_ptr(), ptr(dx), ptr(dy), ptr(ws), N, C, H, W,
             Wh, K, stream_ptr())
        return (dx, dy) + (None,) * 5


def frc(a, b, k_min=1, k_max=None, eps=1e-16, per_image=False):
    """The Fourier ring correlation index of a, b (N,C,H,W) fp32 on one GPU, 2 <= H, W <= 1024, with gradients to both images: with
    ``F = fft2(a)``, ``G = fft2(b)`` and the rings of ``radial_bins(H, W)``, ``r_k = Nk / sqrt(Xk Yk + eps)`` from the ring means ``Nk``
    of ``Re(F conj G) / (HW)``, ``Xk`` of ``|F|^2 / (HW)`` and ``Yk`` of ``|G|^2 / (HW)`` (in double); the index of an image is the mean
    of ``r_k`` over c and ``k_min <= k <= k_max``.  0-dim, the batch mean, or (N,) with ``per_image``; the loss is ``1 - frc``.
    ``k_min = 1`` drops DC; ``k_max = None`` is the Nyquist ring ``min(H, W) // 2``.  In [-1, 1], 1 for identical images, and unchanged
    by a gain on either image.  A ring with ``Xk Yk = 0`` contributes ``r_k = 0`` with finite gradients.  The spectra of both images
    are kept when either needs a gradient, nothing otherwise; no double backward.  Bit-reproducible, ``frc(a, b) == frc(b, a)`` bit
    for bit, always exact fp32 (csrc/spectral.hip)."""
    k_min, k_max, eps = check_frc_params(k_min, k_max, eps)
    _check_frc_operands("frc", a, b)
    k_min, k_max, _ = frc_band(a.shape[2], a.shape[3], k_min, k_max)
    save = torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)          # grad mode is off inside Function.forward
    return _FRC.apply(a, b, k_min, k_max, eps, bool(per_image), save)


def frc_curve(a, b, eps=1e-16):
    """The Fourier ring correlation curve of a, b (N,C,H,W) fp32 on one GPU: ``r_k`` of ``frc`` at every ring of
    ``radial_bins(H, W)``, (N, C, K) fp32.  An evaluation output: it carries no gradient."""
    _, _, eps = check_frc_params(eps=eps)
    _check_frc_operands("frc_curve", a, b)
    with torch.no_grad():
        return frc_forward(a.detach(), b.detach(), 0, 0, eps)[2]


def frc_half_bit(H, W):
    """The half-bit threshold curve of van Heel & Schatz (2005) for the rings of ``radial_bins(H, W)``, float64 (K,):
    ``T_k = (0.2071 + 1.9102 / sqrt(cnt_k)) / (1.2071 + 0.9102 / sqrt(cnt_k))``."""
    s = radial_bins(H, W)[1].double().sqrt()
    return (0.2071 + 1.9102 / s) / (1.2071 + 0.9102 / s)


def check_frc_readout(threshold=1 / 7, smooth=1):
    """``(threshold, smooth)`` of ``frc_cutoff``: a float in (0, 1) or ``"half-bit"``, an odd int in 1..15, or ValueError."""
    if isinstance(threshold, str):
        if threshold != "half-bit":
            raise ValueError("frc_cutoff: threshold must be a float in (0, 1) or \"half-bit\", got %r" % (threshold,))
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0 < threshold < 1:
        raise ValueError("frc_cutoff: threshold must be a float in (0, 1) or \"half-bit\", got %r" % (threshold,))
    else:
        threshold = float(threshold)
    if isinstance(smooth, bool) or not isinstance(smooth, int) or not (1 <= smooth <= FRC_MAX_SMOOTH and smooth % 2 == 1):
        raise ValueError("frc_cutoff: smooth must be an odd int in 1..%d, got %r" % (FRC_MAX_SMOOTH, smooth))
    return threshold, smooth


def frc_cutoff(curve, H, W, threshold=1 / 7, smooth=1, k_min=1, k_max=None):
    """The fractional ring ``k*`` at which a Fourier ring correlation curve (N, C, K) of H x W images falls through a threshold,
    float64 (N, C) on the curve's device.  ``threshold``: a float in (0, 1) (1/7, Nieuwenhuizen et al. 2013), or ``"half-bit"``
    (``frc_half_bit``).  ``smooth``: an odd window 1..15, a moving average over the rings before the read-out whose window shrinks
    symmetrically at the two ends of ``[0, K - 1]``.  With ``d_k = r_k - T_k``, ``k*`` belongs to the first k in ``[k_min, k_max]``
    with ``d_k < 0``: ``k_min`` if that is ``k_min``, else ``(k - 1) + d_{k-1} / (d_{k-1} - d_k)``; without a crossing ``k_max``.
    The cutoff frequency is ``k* / min(H, W)`` cycles per pixel and the resolution ``min(H, W) / k*`` pixels.  Plain torch ops in
    float64: a read-out, not a hot path."""
    k_min, k_max, _ = check_frc_params(k_min, k_max)
    threshold, smooth = check_frc_readout(threshold, smooth)
    k_min, k_max, K = frc_band(H, W, k_min, k_max)
    if not torch.is_tensor(curve) or curve.dim() != 3 or curve.shape[-1] != K or not curve.is_floating_point():
        raise ValueError("frc_cutoff: the curve must be a floating (N, C, %d) tensor for %d x %d, got %s"
                         % (K, H, W, tuple(getattr(curve, "shape", ()))))
    if threshold == "half-bit":
        T = frc_half_bit(H, W).to(curve.device)
    else:
        T = torch.full((K,), threshold, dtype=torch.float64, device=curve.device)
    r = curve.detach().double()
    if smooth > 1:
        k = torch.arange(K, device=r.device)
        half = torch.minimum(torch.minimum(k, K - 1 - k), torch.full_like(k, smooth // 2))
        acc = torch.zeros_like(r)
        for j in range(-(smooth // 2), smooth // 2 + 1):         # neighbours in ascending order, those outside the window as 0
            acc = acc + torch.where(half >= abs(j), r[..., (k + j).clamp(0, K - 1)], torch.zeros_like(r))
        r = acc / (2 * half + 1).double()
    d = r - T
    below = d[..., k_min:k_max + 1] < 0
    first = (below.long().cumsum(-1) == 0).sum(-1)               # rings of the band before the first one below the threshold
    k = first.clamp(max=k_max - k_min) + k_min
    prev = (k - 1).clamp(min=0)
    d0, d1 = d.gather(-1, prev[..., None])[..., 0], d.gather(-1, k[..., None])[..., 0]
    cross = prev.double() + d0 / (d0 - d1)
    out = torch.where(k == k_min, torch.full_like(cross, float(k_min)), cross)
    return torch.where(first > k_max - k_min, torch.full_like(cross, float(k_max)), out)


# ----------------------------------------------------------------------------------------
# phase-correlation registration and the Fourier shift (csrc/spectral.hip, fifth section)
# ----------------------------------------------------------------------------------------
PCORR_MAX_UPSAMPLE = 100


def check_pcorr_params(H, W, upsample=10, max_shift=None, k_max=None, eps=1e-16, normalization="phase"):
    """``(upsample, (max_y, max_x), k_max, eps, normalize)`` of ``phase_correlation`` for H x W images, or ValueError: ``upsample`` an
    int in 1..100; ``max_shift`` None (half the side), an int or a pair of ints, each in ``0..side // 2``; ``k_max`` None (every ring)
    or an int in ``0..K - 1`` of ``radial_bins(H, W)``; ``eps`` finite and >= 0; ``normalization`` ``"phase"`` or None."""
    if isinstance(upsample, bool) or not isinstance(upsample, int) or not 1 <= upsample <= PCORR_MAX_UPSAMPLE:
        raise ValueError("phase_correlation: upsample must be an int in 1..%d, got %r" % (PCORR_MAX_UPSAMPLE, upsample))
    if max_shift is None:
        max_shift = (H // 2, W // 2)
    elif isinstance(max_shift, int) and not isinstance(max_shift, bool):
        max_shift = (max_shift, max_shift)
    try:
        my, mx = max_shift
    except (TypeError, ValueError):
        raise ValueError("phase_correlation: max_shift must be None, an int or a pair of ints, got %r" % (max_shift,))
    for m, side in ((my, H), (mx, W)):
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= side // 2:
            raise ValueError("phase_correlation: max_shift must lie in 0..side // 2 = (%d, %d), got %r" % (H // 2, W // 2, max_shift))
    K = int(radial_bins(H, W)[1].numel())
    if k_max is None:
        k_max = K - 1
    elif isinstance(k_max, bool) or not isinstance(k_max, int) or not 0 <= k_max <= K - 1:
        raise ValueError("phase_correlation: k_max must be None or an int in 0..%d (a %d x %d spectrum has %d rings), got %r"
                         % (K - 1, H, W, K, k_max))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps >= 0):
        raise ValueError("phase_correlation: eps must be a finite number >= 0, got %r" % (eps,))
    if normalization not in ("phase", None):
        raise ValueError("phase_correlation: normalization must be \"phase\" or None, got %r" % (normalization,))
    return upsample, (my, mx), k_max, float(eps), normalization == "phase"


def _check_pcorr_shapes(what, a, b):
    """What the parameter checks need of the operands, before them: two (N,C,H,W) fp32 tensors of one shape with legal sides."""
    for x in (a, b):
        if not torch.is_tensor(x) or x.dim() != 4:
            raise _lib.KernelError("%s operands must be (N,C,H,W) tensors, got %s" % (what, tuple(getattr(x, "shape", ()))))
        if x.dtype != torch.float32:
            raise _lib.KernelError("%s operands must be fp32, got %s" % (what, x.dtype))
        if not (2 <= x.shape[2] <= SPROF_MAX_SIDE and 2 <= x.shape[3] <= SPROF_MAX_SIDE):
            raise _lib.KernelError("%s needs 2 <= H, W <= %d, got %s" % (what, SPROF_MAX_SIDE, tuple(x.shape)))
    if a.shape != b.shape:
        raise _lib.KernelError("%s operands must have one shape: %s vs %s" % (what, tuple(a.shape), tuple(b.shape)))


def _pcorr_launch(a, b, upsample, max_shift, k_max, eps, normalize, want_shift, want_surface):
    a, b = _c(a.detach()), _c(b.detach())
    N, C, H, W = a.shape
    tab_h, half_w, K, Wh, _, _, _, binmap = sprof_tables(H, W, a.device)
    dev = a.device
    n = _lib.load().faoctasr_pcorr_workspace_floats(N, C, H, W, Wh, K, upsample)
    if n < 0:
        raise _lib.KernelError("faoctasr_pcorr_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=dev)               # scratch of this call: free again behind it on the stream
    shift = torch.empty((N, 2), dtype=torch.float32, device=dev) if want_shift else None
    peak = torch.empty(N, dtype=torch.float32, device=dev) if want_shift else None
    surface = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_surface else None
    call("pcorr_fwd", ptr(a), ptr(b), ptr(tab_h), ptr(half_w), binmap.data_ptr(), eps, k_max, int(normalize), upsample, max_shift[0],
         max_shift[1], ptr(shift), ptr(peak), ptr(surface), ptr(ws), N, C, H, W, Wh, K, stream_ptr())
    return shift, peak, surface


def phase_correlation_surface(a, b, k_max=None, eps=1e-16, normalization="phase"):
    """The phase-correlation surface of a, b (N,C,H,W) fp32 on one GPU, (N, H, W): ``sum_c Re ifft2(Rn)`` of ``phase_correlation``.  Its
    maximum lies at ``d`` when ``b(p) = a(p - d)``.  No gradient."""
    _check_pcorr_shapes("phase_correlation_surface", a, b)
    _, _, k_max, eps, normalize = check_pcorr_params(a.shape[2], a.shape[3], 1, None, k_max, eps, normalization)
    _check_frc_operands("phase_correlation_surface", a, b)
    with torch.no_grad():
        return _pcorr_launch(a, b, 1, (0, 0), k_max, eps, normalize, False, True)[2]


def phase_correlation(a, b, upsample=10, max_shift=None, k_max=None, eps=1e-16, normalization="phase"):
    """The translation between a and b (N,C,H,W) fp32 on one GPU, 2 <= H, W <= 1024, by phase correlation (Kuglin & Hines 1975) with
    the upsampled-DFT refinement of Guizar-Sicairos, Thurman & Fienup (2008): ``(shift (N, 2) fp32, peak (N,) fp32)``, one shift
    ``(d_y, d_x)`` per sample for all its channels.  With ``F = fft2(a)``, ``G = fft2(b)``: ``R = G conj(F) / (HW)``,
    ``Rn = R / sqrt(|R|^2 + eps)`` (``normalization="phase"``) or ``R`` (None), zero in every ring of ``radial_bins(H, W)`` above
    ``k_max``; the surface is ``sum_c Re ifft2(Rn)``.  Its first maximum in row-major order with ``|d_y| <= max_shift[0]``,
    ``|d_x| <= max_shift[1]`` is the coarse peak (positions > H//2, > W//2 wrap negative).  ``upsample = U > 1`` evaluates the inverse
    transform at ``T = ceil(1.5 U)`` offsets ``(j - T//2) / U`` per axis around it and takes the first maximum there; the shift is a
    multiple of ``1 / U``.  ``peak`` is the winning value, in (0, 1] under phase normalisation: a confidence.
    SIGN: the shift is ``d`` when ``b(p) = a(p - d)``: ``b = torch.roll(a, (3, -2), (-2, -1))`` gives ``(3, -2)``, and
    ``fourier_shift(b, -shift)`` lies on ``a``.  ``skimage.registration.phase_cross_correlation(a, b)`` returns ``-d``.
    No gradient.  No host synchronisation: capturable, bit-reproducible, always exact fp32 (csrc/spectral.hip)."""
    _check_pcorr_shapes("phase_correlation", a, b)
    upsample, max_shift, k_max, eps, normalize = check_pcorr_params(a.shape[2], a.shape[3], upsample, max_shift, k_max, eps, normalization)
    _check_frc_operands("phase_correlation", a, b)
    with torch.no_grad():
        shift, peak, _ = _pcorr_launch(a, b, upsample, max_shift, k_max, eps, normalize, True, False)
    return shift, peak


def _fourier_shift_launch(x, shift, sign):
    x = _c(x)
    N, C, H, W = x.shape
    tab_h, half_w = dft_tables(H, x.device), sprof_half_tables(W, x.device)
    n = _lib.load().faoctasr_fourier_shift_workspace_floats(N, C, H, W)
    if n < 0:
        raise _lib.KernelError("faoctasr_fourier_shift_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)          # scratch of this call: free again behind it on the stream
    out = torch.empty_like(x)
    call("fourier_shift", ptr(x), ptr(shift), sign, ptr(tab_h), ptr(half_w), ptr(out), ptr(ws), N, C, H, W, stream_ptr())
    return out


class _FourierShift(Function):
    @staticmethod
    def forward(ctx, x, shift):
        ctx.save_for_backward(shift)
        return _fourier_shift_launch(x, shift, 1.0)

    @staticmethod
    def backward(ctx, g):
        shift, = ctx.saved_tensors
        return _fourier_shift_launch(g, shift, -1.0), None             # the transpose of the shift by d is the shift by -d


def fourier_shift(x, shift):
    """``Re ifft2(fft2(x) exp(-2 pi i (f_u d_y + f_v d_x)))`` of x (N,C,H,W) fp32 on one GPU, 2 <= H, W <= 1024, ``f`` of
    ``numpy.fft.fftfreq``: the content moves by ``+d`` (periodically), to a fraction of a pixel; an integer ``d`` is
    ``torch.roll(x, d, (-2, -1))`` up to rounding.  ``shift``: an (N, 2) fp32 tensor on x's device, one ``(d_y, d_x)`` per sample as
    ``phase_correlation`` returns it, or a pair of floats for the whole batch.  Differentiable in x (the backward is the shift by
    ``-d``; only ``shift`` is kept); there is no gradient to ``shift``: asking for one raises (the open follow-up).  Always exact fp32
    (csrc/spectral.hip)."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32:
        raise _lib.KernelError("fourier_shift: x must be an (N,C,H,W) fp32 tensor, got %s %s" % (tuple(getattr(x, "shape", ())), getattr(x, "dtype", None)))
    N = x.shape[0]
    if not torch.is_tensor(shift):
        try:
            dy, dx = (float(v) for v in shift)
        except (TypeError, ValueError):
            raise ValueError("fourier_shift: shift must be an (N, 2) tensor or a pair of floats, got %r" % (shift,))
        if not (math.isfinite(dy) and math.isfinite(dx)):
            raise ValueError("fourier_shift: shift must be finite, got %r" % (shift,))
    _check_sprof_operands("fourier_shift", x)
    if torch.is_tensor(shift):
        if shift.requires_grad and torch.is_grad_enabled():
            raise _lib.KernelError("fourier_shift has no gradient with respect to the shift (an open follow-up); detach it")
        if shift.shape != (N, 2) or shift.dtype != torch.float32 or shift.device != x.device:
            raise _lib.KernelError("fourier_shift: shift must be an (N, 2) = (%d, 2) fp32 tensor on %s, got %s %s on %s"
                                   % (N, x.device, tuple(shift.shape), shift.dtype, shift.device))
        shift = _c(shift.detach())
    else:
        shift = torch.tensor([[dy, dx]], dtype=torch.float32).expand(N, 2).contiguous().to(x.device)
    return _FourierShift.apply(x, shift)


# ----------------------------------------------------------------------------------------
# differentiable mutual information (Gaussian Parzen windows, soft joint histogram; csrc/mi.hip)
# ----------------------------------------------------------------------------------------
MI_MAX_BINS = 64


def check_mi_params(bins, value_range, sigma_ratio, eps):
    """``(bins, (lo, hi), sigma_ratio, eps)`` of the mutual-information op as an int and floats, or ValueError."""
    if isinstance(bins, bool) or not isinstance(bins, int) or not 2 <= bins <= MI_MAX_BINS:
        raise ValueError("mutual information: bins must be an int in [2, %d], got %r" % (MI_MAX_BINS, bins))
    try:
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError("mutual information: value_range must be a (lo, hi) pair, got %r" % (value_range,))
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError("mutual information: value_range must be finite with hi > lo, got %r" % ((lo, hi),))
    sigma_ratio, eps = float(sigma_ratio), float(eps)
    if not (math.isfinite(sigma_ratio) and sigma_ratio > 0.0):
        raise ValueError("mutual information: sigma_ratio must be finite and > 0, got %r" % sigma_ratio)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("mutual information: eps must be finite and > 0, got %r" % eps)
    return bins, (lo, hi), sigma_ratio, eps


class _MutualInformation(Function):
    @staticmethod
    def forward(ctx, x, y, bins, lo, hi, sigma_ratio, eps, normalized, per_image, save):
        x, y = _c(x), _c(y)
        N, C, H, W = x.shape
        n = _lib.load().faoctasr_mi_workspace_floats(N, C, H, W, bins)
        if n < 0:
            raise _lib.KernelError("faoctasr_mi_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = torch.empty(n, dtype=torch.float32, device=x.device)        # scratch of this call: free again behind it on the stream
        out = torch.empty((N,) if per_image else (), dtype=torch.float32, device=x.device)
        # dS/dP per plane (bins x bins): all a backward needs besides x and y; stored only when one can follow (``save``)
        table = torch.empty(N * C * bins * bins, dtype=torch.float32, device=x.device) if save else None
        call("mi_fwd", ptr(x), ptr(y), ptr(out), ptr(table), ptr(ws), N, C, H, W, bins, lo, hi, sigma_ratio, eps, int(normalized),
             int(per_image), stream_ptr())
        if save:
            ctx.save_for_backward(x, y, table)
        ctx.cfg = (bins, lo, hi, sigma_ratio, int(per_image), N, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, table = ctx.saved_tensors
        bins, lo, hi, sigma_ratio, per_image, N, C, H, W = ctx.cfg
        g = _c(g)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        call("mi_bwd", ptr(g), ptr(x), ptr(y), ptr(table), ptr(dx), ptr(dy), N, C, H, W, bins, lo, hi, sigma_ratio, per_image, stream_ptr())
        return (dx, dy) + (None,) * 8


def mutual_information(x, y, bins=32, value_range=(-1., 1.), sigma_ratio=1.0, eps=1e-6, normalized=False, per_image=False):
    """The differentiable mutual information of x and y (N,C,H,W) fp32 on one GPU, with gradients to both inputs.  Per (n, c)
    plane, with ``K = bins``, ``d = (hi - lo) / K``, centres ``c_k = lo + (k + 1/2) d`` and ``sigma = sigma_ratio * d``:
    ``Wa[p, k] = softmax_k(-(x_p - c_k)^2 / (2 sigma^2))`` (Gaussian Parzen windows; any finite value, inside the range or not),
    ``Wb`` likewise from y, ``P = Wa^T Wb / (H W)``, ``pa`` / ``pb`` its row / column sums, ``H(q) = -sum q log(q + eps)`` and
    ``MI = Ha + Hb - Hab``, or with ``normalized`` ``NMI = (Ha + Hb) / Hab``.  The result is the mean over all planes as a 0-dim
    tensor, or with ``per_image`` the ``(N,)`` means over c.  Invariant to any invertible intensity map of either image (up to the
    binning), which makes it the structure-preservation measure between images of DIFFERENT domains.  Nothing of size pixels x
    bins is stored (csrc/mi.hip): the weights are contracted on the exact-f32 MFMA as they are formed and recomputed in the
    backward, which needs x, y and one K x K table per plane.  Bit-reproducible, symmetric in (x, y) bit for bit, always exact
    fp32 (``conv_precision`` does not apply); no double backward."""
    bins, (lo, hi), sigma_ratio, eps = check_mi_params(bins, value_range, sigma_ratio, eps)
    if not (torch.is_tensor(x) and torch.is_tensor(y)) or x.dim() != 4 or x.shape != y.shape:
        raise _lib.KernelError("mutual_information operands must be (N,C,H,W) tensors of one shape: %s vs %s"
                               % (tuple(getattr(x, "shape", ())), tuple(getattr(y, "shape", ()))))
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise _lib.KernelError("mutual_information operands must be fp32, got %s and %s" % (x.dtype, y.dtype))
    if not (x.is_cuda and y.is_cuda) or x.device != y.device:
        raise _lib.KernelError("mutual_information runs as HIP kernels on one GPU; got devices %s and %s" % (x.device, y.device))
    if x.numel() == 0 or x.shape[0] * x.shape[1] > 65535:
        raise _lib.KernelError("mutual_information needs a non-empty batch of at most 65535 planes, got %s" % (tuple(x.shape),))
    save = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)         # grad mode is off inside Function.forward
    return _MutualInformation.apply(x, y, bins, lo, hi, sigma_ratio, eps, bool(normalized), bool(per_image), save)


# ----------------------------------------------------------------------------------------
# total-variation loss (model.py:17-33)
# ----------------------------------------------------------------------------------------
class _TVLoss(Function):
    @staticmethod
    def forward(ctx, x, weight):
        x = _c(x)
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[2] < 2 or x.shape[3] < 2:
            raise _lib.KernelError("tv_loss operand must be a (B,C,H,W) fp32 tensor with H, W >= 2, got %s %s" % (tuple(x.shape), x.dtype))
        B, C, H, W = x.shape
        n = _lib.load().faoctasr_tv_loss_workspace_floats(B, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_tv_loss_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ws = _lib.workspace(x.device, n)              # per stream: the partial sums are consumed by the same call's second launch
        call("tv_loss_fwd", ptr(x), ptr(out), ptr(ws), B, C, H, W, weight, stream_ptr())
        ctx.save_for_backward(x)
        ctx.weight = weight
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        dx = torch.empty_like(x)
        call("tv_loss_bwd", ptr(x), ptr(_c(g)), ptr(dx), B, C, H, W, ctx.weight, stream_ptr())
        return dx, None


def tv_loss(x, weight=1.0):
    """``TVLoss(weight)(x)`` of model.py:17-33 for x (B,C,H,W), H, W >= 2, as a 0-dim fp32 tensor with a gradient to ``x``:
    ``weight * 2 * (sum of squared vertical differences / (C (H-1) W) + sum of squared horizontal differences / (C H (W-1))) / B``.
    One pass over ``x`` and a fixed-order reduction forward, one stencil kernel backward (csrc/tv.hip); bit-reproducible, always
    exact fp32 (``conv_precision`` does not apply)."""
    return _TVLoss.apply(x, float(weight))


# ----------------------------------------------------------------------------------------
# losses and the discriminator head
# ----------------------------------------------------------------------------------------
LOSS_MSE, LOSS_L1, LOSS_BCE_LOGITS = 0, 1, 2


class _Loss(Function):
    @staticmethod
    def forward(ctx, a, b, kind, scale):
        a, b = _c(a), _c(b)
        if a.shape != b.shape:
            raise _lib.KernelError("loss operands differ in shape: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = _lib.workspace(a.device, 1024)
        call("loss_fwd", ptr(a), ptr(b), ptr(out), a.numel(), kind, scale, ptr(ws), stream_ptr())
        ctx.save_for_backward(a, b)
        ctx.cfg = (kind, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        kind, scale = ctx.cfg
        g = _c(g)
        da = db = None
        st = stream_ptr()
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(a)
            call("loss_bwd", ptr(a), ptr(b), ptr(g), ptr(da), a.numel(), kind, scale, 0, st)
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(b)
            call("loss_bwd", ptr(a), ptr(b), ptr(g), ptr(db), a.numel(), kind, scale, 1, st)
        return da, db, None, None


def mse_loss(a, b, weight=1.0):
    return _Loss.apply(a, b, LOSS_MSE, float(weight) / a.numel())


def l1_loss(a, b, weight=1.0):
    return _Loss.apply(a, b, LOSS_L1, float(weight) / a.numel())


def bce_with_logits(inp, target, weight=1.0):
    """torch.nn.BCEWithLogitsLoss()(inp, target); the gradient w.r.t. ``target`` is -inp/N (train.py:230-231)."""
    return _Loss.apply(inp, target, LOSS_BCE_LOGITS, float(weight) / inp.numel())


class _MeanMix(Function):
    @staticmethod
    def forward(ctx, a, b, wa, wb):
        if a.dim() < 1 or b.dim() < 1 or a.shape[0] != b.shape[0]:
            raise _lib.KernelError("mean_mix operands differ in batch size: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        a, b = _c(a), _c(b)
        N = a.shape[0]
        La, Lb = a.numel() // N, b.numel() // N
        out = torch.empty(N, dtype=torch.float32, device=a.device)
        call("mean_mix_fwd", ptr(a), ptr(b), ptr(out), N, La, Lb, wa, wb, stream_ptr())
        ctx.cfg = (a.shape, b.shape, wa, wb)
        return out

    @staticmethod
    def backward(ctx, g):
        sa, sb, wa, wb = ctx.cfg
        g = _c(g)
        N = sa[0]
        da = torch.empty(sa, dtype=torch.float32, device=g.device)
        db = torch.empty(sb, dtype=torch.float32, device=g.device)
        call("mean_mix_bwd", ptr(g), ptr(da), ptr(db), N, da.numel() // N, db.numel() // N, wa, wb, stream_ptr())
        return da, db, None, None


def mean_mix(a, b, wa=0.7, wb=0.3):
    """flatten(wa * global_avg_pool(a) + wb * global_avg_pool(b)) -- model.py:158-164."""
    return _MeanMix.apply(a, b, float(wa), float(wb))


# ----------------------------------------------------------------------------------------
# SSIM
# ----------------------------------------------------------------------------------------
class _SSIM(Function):
    @staticmethod
    def forward(ctx, a, b, size_average):
        a, b = _c(a), _c(b)
        N, C, H, W = a.shape
        sums = torch.empty(N, dtype=torch.float32, device=a.device)
        call("ssim_fwd", ptr(a), ptr(b), ptr(sums), N, C, H, W, stream_ptr())
        ctx.save_for_backward(a, b)
        ctx.size_average = size_average
        # the final division of N (or 1) numbers is host-side plumbing on a tiny tensor
        return sums.sum() / (N * C * H * W) if size_average else sums / (C * H * W)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        N, C, H, W = a.shape
        g = _c(g).reshape(-1)
        scale = 1.0 / (N * C * H * W) if ctx.size_average else 1.0 / (C * H * W)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        call("ssim_bwd", ptr(a), ptr(b), ptr(g), g.numel(), scale, ptr(da), ptr(db), N, C, H, W, stream_ptr())
        return da, db, None


def ssim(a, b, size_average=True):
    return _SSIM.apply(a, b, bool(size_average))


# ----------------------------------------------------------------------------------------
# multi-scale SSIM (csrc/msssim.hip): the contrast-structure factor at every dyadic scale, the luminance factor at the coarsest
# ----------------------------------------------------------------------------------------
MSSSIM_MAX_LEVELS = 5
#: Wang, Simoncelli & Bovik 2003; the first M are used as they stand
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _msssim_check_scalars(levels, weights, data_range):
    """The refusals of ``ms_ssim`` that concern no tensor; returns the weights as floats."""
    if isinstance(levels, bool) or int(levels) != levels or not 1 <= levels <= MSSSIM_MAX_LEVELS:
        raise ValueError("levels must be an integer 1..%d, got %r" % (MSSSIM_MAX_LEVELS, levels))
    levels = int(levels)
    w = MSSSIM_WEIGHTS[:levels] if weights is None else tuple(float(v) for v in weights)
    if len(w) != levels:
        raise ValueError("weights lists one weight per scale: %d entries for levels = %d" % (len(w), levels))
    if not all(v > 0 and v < float("inf") for v in w):
        raise ValueError("every weight must be positive and finite, got %r" % (w,))
    if not (data_range > 0 and data_range < float("inf")):
        raise ValueError("data_range must be positive and finite, got %r" % (data_range,))
    return w


def _msssim_check(a, b, levels, weights, data_range):
    """Every refusal of ``ms_ssim``, the device check last; returns the weights as floats."""
    w = _msssim_check_scalars(levels, weights, data_range)
    levels = len(w)
    for t, what in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError("%s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("the index takes non-empty images, got %s" % (tuple(a.shape),))
    if min(a.shape[2], a.shape[3]) < 2 ** (levels - 1):
        raise ValueError("a %d x %d image leaves scale %d empty: every side must be at least %d"
                         % (a.shape[2], a.shape[3], levels, 2 ** (levels - 1)))
    for t, what in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if a.device != b.device:
        raise ValueError("a and b must be on one device, got %s and %s" % (a.device, b.device))
    return w


class _MSSSIM(Function):
    """``apply(a, b, weights, C1, C2, per_image, want_a, want_b) -> MS``: one ``msssim_scale_fwd`` per scale and ``msssim_final``
    forward; where an input needs a gradient the pooled pairs of scales 2..M and the coefficient table are saved, and the backward is
    one ``msssim_scale_bwd`` per scale, coarsest first, reading the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, weights, C1, C2, per_image, want_a, want_b):
        N, C, H, W = a.shape
        M, dev = len(weights), a.device
        n = _lib.load().faoctasr_msssim_workspace_floats(N * C, H, W, M)
        if n < 0:
            raise _lib.KernelError("faoctasr_msssim_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "msssim")                 # per stream: consumed by the same call's last launch
        pairs = [(a, b)]
        for j in range(M):
            pa = pb = None
            if j < M - 1:
                pa = torch.empty((N, C, H >> (j + 1), W >> (j + 1)), dtype=torch.float32, device=dev)
                pb = torch.empty_like(pa)
                pairs.append((pa, pb))
            call("msssim_scale_fwd", ptr(pairs[j][0]), ptr(pairs[j][1]), ptr(pa), ptr(pb), ws.data_ptr(), N * C, H, W, M, j, C1, C2, stream_ptr())
        want = want_a or want_b
        coef = torch.empty((M, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = torch.empty((), dtype=torch.float32, device=dev)
        call("msssim_final", ws.data_ptr(), N, C, H, W, M, ctypes.cast((ctypes.c_double * M)(*weights), ctypes.c_void_p), int(not per_image),
             ptr(out_image), ptr(out_mean), ptr(coef), stream_ptr())
        ctx.cfg = (M, C1, C2, want_a, want_b)
        if want:
            ctx.save_for_backward(coef, *(t for p in pairs for t in p))
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        M, C1, C2, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 8
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("ms_ssim's forward ran without gradients enabled for this input: nothing was saved")
        coef, *flat = ctx.saved_tensors
        N, C, H, W = flat[0].shape
        g = _c(g).reshape(-1)
        da = db = None
        for j in range(M - 1, -1, -1):
            aj, bj = flat[2 * j], flat[2 * j + 1]
            dca, dcb = da, db
            da = torch.empty_like(aj) if need_a else None
            db = torch.empty_like(bj) if need_b else None
            call("msssim_scale_bwd", ptr(aj), ptr(bj), ptr(coef), ptr(g), g.numel(), ptr(dca), ptr(dcb), ptr(da), ptr(db), N, C, H, W, M, j,
                 C1, C2, stream_ptr())
        return (da, db) + (None,) * 6


def ms_ssim(a, b, levels=5, weights=None, data_range=1.0, per_image=False):
    """Multi-scale SSIM (Wang, Simoncelli & Bovik 2003) of two images ``(N, C, H, W)``: scale 1 is the input and scale j + 1 is
    ``avg_pool2d(scale j, 2)``; with the moments of ``ssim`` (11-tap sigma-1.5 Gaussian, zero padding 5) at every scale

        cs_p = (2 s12 + C2) / (s11 + s22 + C2),   l_p = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1),   C1 = (0.01 L)^2, C2 = (0.03 L)^2,

    ``F_j[n]`` the mean of cs_p over image n at scale j < M and of l_p cs_p at scale M = ``levels``, the score is
    ``MS[n] = prod_j max(F_j[n], 0)^w_j``: the mean over n as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``.  ``weights``
    defaults to the first M of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), not renormalised; ``levels=1, weights=(1,)`` is ``ssim``.
    Where a factor is <= 0 the image's score is 0 and its gradient exactly zero.  Gradients to both images; M + 1 launches of
    csrc/msssim.hip forward and M backward; under ``no_grad``, or for inputs that need no gradient, nothing is saved.
    ``MS(x, x) == 1`` with zero gradients and ``MS(x, y) == MS(y, x)`` hold bit for bit; runs are bit-reproducible.  Every side
    must be at least ``2^(M - 1)``.  fp32, no double backward."""
    w = _msssim_check(a, b, levels, weights, data_range)
    L = float(data_range)
    grad = torch.is_grad_enabled()
    return _MSSSIM.apply(a.contiguous(), b.contiguous(), w, (0.01 * L) ** 2, (0.03 * L) ** 2, bool(per_image), grad and a.requires_grad,
                         grad and b.requires_grad)


# ----------------------------------------------------------------------------------------
# HaarPSI (csrc/haarpsi.hip): Haar coefficients of the half-resolution pair, edge-weighted logistic of the local similarity
# ----------------------------------------------------------------------------------------
def _haarpsi_check_scalars(c, alpha, value_range):
    """The refusals of ``haarpsi`` that concern no tensor; returns ``(c, alpha, lo, hi)`` as floats."""
    for v, what in ((c, "c"), (alpha, "alpha")):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s must be a number, got %r" % (what, v))
        if not (v > 0 and v < float("inf")):
            raise ValueError("%s must be positive and finite, got %r" % (what, v))
    try:
        lo, hi = value_range
    except (TypeError, ValueError):
        raise TypeError("value_range must be a pair (lo, hi), got %r" % (value_range,)) from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("value_range must hold two numbers, got %r" % (value_range,))
    if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite with hi > lo, got %r" % (value_range,))
    return float(c), float(alpha), float(lo), float(hi)


def _haarpsi_check(a, b, c, alpha, value_range):
    """Every refusal of ``haarpsi``, the device check last; returns ``(c, alpha, lo, hi)``."""
    cfg = _haarpsi_check_scalars(c, alpha, value_range)
    for t, what in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor, got %s" % (what, t.dtype))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("the index takes non-empty images, got %s" % (tuple(a.shape),))
    if min(a.shape[2], a.shape[3]) < 2:
        raise ValueError("every side must be at least 2, got %d x %d" % (a.shape[2], a.shape[3]))
    for t, what in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if a.device != b.device:
        raise ValueError("a and b must be on one device, got %s and %s" % (a.device, b.device))
    return cfg


class _HaarPSI(Function):
    """``apply(a, b, c, alpha, lo, hi, per_image, want_a, want_b) -> HaarPSI``: ``haarpsi_index`` and ``haarpsi_final`` forward; where
    an input needs a gradient the two images and the (2, N) factor table are saved, and the backward is one ``haarpsi_grad``, which
    reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, c, alpha, lo, hi, per_image, want_a, want_b):
        N, C, H, W = a.shape
        dev = a.device
        n = _lib.load().faoctasr_haarpsi_workspace_floats(N * C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_haarpsi_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "haarpsi")                # per stream: consumed by the same call's second launch
        call("haarpsi_index", ptr(a), ptr(b), ws.data_ptr(), N * C, H, W, lo, hi, c, alpha, stream_ptr())
        want = want_a or want_b
        fac = torch.empty((2, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = torch.empty((), dtype=torch.float32, device=dev)
        call("haarpsi_final", ws.data_ptr(), N, C, H, W, alpha, int(not per_image), ptr(out_image), ptr(out_mean), ptr(fac), stream_ptr())
        ctx.cfg = (c, alpha, lo, hi, want_a, want_b)
        if want:
            ctx.save_for_backward(a, b, fac)
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        c, alpha, lo, hi, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 9
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("haarpsi's forward ran without gradients enabled for this input: nothing was saved")
        a, b, fac = ctx.saved_tensors
        N, C, H, W = a.shape
        g = _c(g).reshape(-1)
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        call("haarpsi_grad", ptr(a), ptr(b), ptr(fac), ptr(g), g.numel(), ptr(da), ptr(db), N, C, H, W, lo, hi, c, alpha, stream_ptr())
        return (da, db) + (None,) * 7


def haarpsi(a, b, c=30.0, alpha=4.2, value_range=(-1., 1.), per_image=False):
    """The Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok & Wiegand 2018) of two images ``(N, C, H, W)``,
    every channel an independent grey plane pooled inside its image.  With ``u = (x - lo) 255 / (hi - lo)``, ``u2`` its 2 x 2 mean at
    every second pixel (samples beyond the image 0, divisor 4), ``g^o_k`` the horizontal and vertical Haar coefficients of ``u2`` at
    the scales 2, 4, 8 (``2^-k`` times the difference of the two half-window sums, zero outside the map), ``a_k = |g^o_k(a)|`` and
    ``b_k = |g^o_k(b)|``:

        S_o = 1/2 sum_{k = 1, 2} (2 a_k b_k + c) / (a_k^2 + b_k^2 + c),   W_o = max(a_3, b_3),
        r[n] = sum sigmoid(alpha S_o) W_o / sum W_o,   HaarPSI[n] = (log(r / (1 - r)) / alpha)^2,

    the mean over n as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``; 1 for identical images, and 1 with zero gradients where
    neither image has any structure at the coarse scale.  The loss is ``1 - haarpsi``.  Gradients to both images (``d|g|/dg`` is
    ``sign(g)`` with ``sign(0) = 0``; in ``max`` the gradient goes to the larger side, at equality to ``a``).  Two launches of
    csrc/haarpsi.hip forward and one backward; under ``no_grad``, or for inputs that need no gradient, nothing is saved, otherwise
    the two images and a (2, N) table.  ``haarpsi(x, y) == haarpsi(y, x)`` bit for bit with swapped gradients; runs are
    bit-reproducible.  Every side must be at least 2.  fp32, grey planes only (no YIQ chroma term), no double backward."""
    c, alpha, lo, hi = _haarpsi_check(a, b, c, alpha, value_range)
    grad = torch.is_grad_enabled()
    return _HaarPSI.apply(a.contiguous(), b.contiguous(), c, alpha, lo, hi, bool(per_image), grad and a.requires_grad, grad and b.requires_grad)


# ----------------------------------------------------------------------------------------
# Local normalised cross-correlation (csrc/lncc.hip): the squared correlation coefficient inside a sliding box window
# ----------------------------------------------------------------------------------------
LNCC_MAX_WIN = 15


def _lncc_check_scalars(win, eps):
    """The refusals of ``lncc`` that concern no tensor; returns ``(win, eps)`` as an int and a float."""
    if isinstance(win, bool) or not isinstance(win, int):
        raise TypeError("win must be an integer, got %r" % (win,))
    if not 3 <= win <= LNCC_MAX_WIN or win % 2 == 0:
        raise ValueError("win must be odd in 3..%d, got %r" % (LNCC_MAX_WIN, win))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise TypeError("eps must be a number, got %r" % (eps,))
    if not (eps > 0 and eps < float("inf")):
        raise ValueError("eps must be positive and finite, got %r" % (eps,))
    return int(win), float(eps)


def _lncc_check(a, b, win, eps):
    """Every refusal of ``lncc``, the device check last; returns ``(win, eps)``."""
    cfg = _lncc_check_scalars(win, eps)
    for t, what in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor, got %s" % (what, t.dtype))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.numel() == 0:
        raise ValueError("the index takes non-empty images, got %s" % (tuple(a.shape),))
    for t, what in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if a.device != b.device:
        raise ValueError("a and b must be on one device, got %s and %s" % (a.device, b.device))
    return cfg


class _LNCC(Function):
    """``apply(a, b, win, eps, per_image, want_a, want_b) -> LNCC``: ``lncc_index`` and ``lncc_final`` forward; where an input needs a
    gradient the two images and the (N,) factor table are saved, and the backward is one ``lncc_grad``, which reads the upstream
    gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, win, eps, per_image, want_a, want_b):
        N, C, H, W = a.shape
        dev = a.device
        n = _lib.load().faoctasr_lncc_workspace_floats(N * C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_lncc_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "lncc")                   # per stream: consumed by the same call's second launch
        call("lncc_index", ptr(a), ptr(b), ws.data_ptr(), N * C, H, W, win, eps, stream_ptr())
        want = want_a or want_b
        fac = torch.empty((N,), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = torch.empty((), dtype=torch.float32, device=dev)
        call("lncc_final", ws.data_ptr(), N, C, H, W, int(not per_image), ptr(out_image), ptr(out_mean), ptr(fac), stream_ptr())
        ctx.cfg = (win, eps, want_a, want_b)
        if want:
            ctx.save_for_backward(a, b, fac)
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        win, eps, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 7
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("lncc's forward ran without gradients enabled for this input: nothing was saved")
        a, b, fac = ctx.saved_tensors
        N, C, H, W = a.shape
        g = _c(g).reshape(-1)
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        call("lncc_grad", ptr(a), ptr(b), ptr(fac), ptr(g), g.numel(), ptr(da), ptr(db), N, C, H, W, win, eps, stream_ptr())
        return (da, db) + (None,) * 5


def lncc(a, b, win=9, eps=1e-5, per_image=False):
    """Local (windowed) normalised cross-correlation of two images ``(N, C, H, W)``: the squared correlation coefficient of the pair
    inside a sliding ``win x win`` box.  With ``n = win^2`` and ``box(t)_p`` the sum of ``t`` over the window centred on ``p`` (samples
    beyond the image count as 0 and the divisor is always ``n``: the zero-padded ``conv2d`` form; the window may be larger than the
    image):

        u = box(a b) - box(a) box(b) / n,   va = box(a a) - box(a)^2 / n,   vb = box(b b) - box(b)^2 / n,
        cc_p = u^2 / (va vb + eps),   LNCC[n] = mean of cc_p over c, y, x,

    the mean over n as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``.  The index is invariant to an affine intensity map of either
    image inside the window; the loss is ``1 - lncc``.  Gradients to both images, nothing is clamped.  Two launches of csrc/lncc.hip
    forward and one backward; under ``no_grad``, or for inputs that need no gradient, nothing is saved, otherwise the two images and
    an (N,) table.  ``lncc(x, y) == lncc(y, x)`` bit for bit with swapped gradients, halving the upstream gradient halves the
    gradients bit for bit, and runs are bit-reproducible.  ``win`` is odd in 3..15.  As in the torch form, ``va`` is a difference of
    two sums: precision falls where the local mean dwarfs the local contrast.  fp32, no double backward."""
    win, eps = _lncc_check(a, b, win, eps)
    grad = torch.is_grad_enabled()
    return _LNCC.apply(a.contiguous(), b.contiguous(), win, eps, bool(per_image), grad and a.requires_grad, grad and b.requires_grad)


# ----------------------------------------------------------------------------------------
# GMSD and multi-scale GMSD (csrc/gmsd.hip): the deviation of the Prewitt gradient-magnitude similarity map
# ----------------------------------------------------------------------------------------
GMSD_MAX_SCALES = 5
#: Zhang, Shen, Wang & Li 2017
MSGMSD_WEIGHTS = (0.096, 0.596, 0.289, 0.019)


def _gmsd_check_scalars(c, value_range, weights=None):
    """The refusals of ``gmsd`` and ``ms_gmsd`` that concern no tensor; returns ``(c, lo, hi, weights)``, floats and a tuple of floats
    (``weights`` None stays None: plain GMSD has none)."""
    if isinstance(c, bool) or not isinstance(c, (int, float)):
        raise TypeError("c must be a number, got %r" % (c,))
    if not (c > 0 and c < float("inf")):
        raise ValueError("c must be positive and finite, got %r" % (c,))
    try:
        lo, hi = value_range
    except (TypeError, ValueError):
        raise TypeError("value_range must be a pair (lo, hi), got %r" % (value_range,)) from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("value_range must hold two numbers, got %r" % (value_range,))
    if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite with hi > lo, got %r" % (value_range,))
    if weights is not None:
        try:
            weights = tuple(weights)
        except TypeError:
            raise TypeError("weights must be a sequence of numbers, got %r" % (weights,)) from None
        for v in weights:
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError("weights must hold numbers, got %r" % (weights,))
        if not 1 <= len(weights) <= GMSD_MAX_SCALES:
            raise ValueError("weights lists one weight per scale, 1..%d of them, got %d" % (GMSD_MAX_SCALES, len(weights)))
        if not all(v >= 0 and v < float("inf") for v in weights):
            raise ValueError("every weight must be finite and >= 0, got %r" % (weights,))
        if not any(v > 0 for v in weights):
            raise ValueError("the weights must not all be zero, got %r" % (weights,))
        weights = tuple(float(v) for v in weights)
    return float(c), float(lo), float(hi), weights


def _gmsd_check(a, b, c, value_range, weights=None):
    """Every refusal of ``gmsd`` (``weights`` None) and ``ms_gmsd``, the device check last; returns ``(c, lo, hi, weights)``."""
    cfg = _gmsd_check_scalars(c, value_range, weights)
    for t, what in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor, got %s" % (what, t.dtype))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.numel() == 0:
        raise ValueError("the index takes non-empty images, got %s" % (tuple(a.shape),))
    least = 2 if cfg[3] is None else 2 ** (len(cfg[3]) - 1)
    if min(a.shape[2], a.shape[3]) < least:
        raise ValueError("every side must be at least %d, got %d x %d" % (least, a.shape[2], a.shape[3]))
    for t, what in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if a.device != b.device:
        raise ValueError("a and b must be on one device, got %s and %s" % (a.device, b.device))
    return cfg


class _GMSD(Function):
    """``apply(a, b, weights, c, lo, hi, per_image, want_a, want_b) -> score``.  ``weights`` None is plain GMSD: one ``gmsd_index`` in the
    pooled form and ``gmsd_final`` forward, one ``gmsd_grad`` backward; saved where an input needs a gradient: the two images and the
    table.  Otherwise MS-GMSD over ``M = len(weights)`` scales: one ``gmsd_index`` per scale, which also writes the next scale's pair
    (a scale of weight 0 takes no workspace and only pools), and ``gmsd_final``; one ``gmsd_grad`` per scale backward, coarsest first;
    saved: additionally the pooled pairs of scales 2..M.  The backward reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, weights, c, lo, hi, per_image, want_a, want_b):
        N, C, H, W = a.shape
        dev = a.device
        pooled = int(weights is None)
        w = (1.0,) if pooled else weights
        M = len(w)
        n = _lib.load().faoctasr_gmsd_workspace_floats(N * C, H, W, M, pooled)
        if n < 0:
            raise _lib.KernelError("faoctasr_gmsd_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "gmsd")                   # per stream: consumed by the same call's last launch
        pairs = [(a, b)]
        for j in range(M):
            pa = pb = None
            if j < M - 1:
                pa = torch.empty((N, C, H >> (j + 1), W >> (j + 1)), dtype=torch.float32, device=dev)
                pb = torch.empty_like(pa)
                pairs.append((pa, pb))
            call("gmsd_index", ptr(pairs[j][0]), ptr(pairs[j][1]), ptr(pa), ptr(pb), ws.data_ptr() if w[j] > 0 else None, N * C, H, W, M, j,
                 pooled, lo, hi, c, stream_ptr())
        want = want_a or want_b
        table = torch.empty((2, M, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = torch.empty((), dtype=torch.float32, device=dev)
        call("gmsd_final", ws.data_ptr(), N, C, H, W, M, pooled, ctypes.cast((ctypes.c_double * M)(*w), ctypes.c_void_p), int(not per_image),
             ptr(out_image), ptr(out_mean), ptr(table), stream_ptr())
        ctx.cfg = (M, pooled, c, lo, hi, want_a, want_b)
        if want:
            ctx.save_for_backward(table, *(t for p in pairs for t in p))
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        M, pooled, c, lo, hi, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 9
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("gmsd's forward ran without gradients enabled for this input: nothing was saved")
        table, *flat = ctx.saved_tensors
        N, C, H, W = flat[0].shape
        g = _c(g).reshape(-1)
        da = db = None
        for j in range(M - 1, -1, -1):
            aj, bj = flat[2 * j], flat[2 * j + 1]
            dca, dcb = da, db
            da = torch.empty_like(aj) if need_a else None
            db = torch.empty_like(bj) if need_b else None
            call("gmsd_grad", ptr(aj), ptr(bj), ptr(table), ptr(g), g.numel(), ptr(dca), ptr(dcb), ptr(da), ptr(db), N, C, H, W, M, j, pooled,
                 lo, hi, c, stream_ptr())
        return (da, db) + (None,) * 7


_GMSD_DOC = """With ``u = (x - lo) / (hi - lo)`` for ``value_range = (lo, hi)``, ``pool(t) = avg_pool2d(t, 2)`` (floor pooling: an odd last
    row or column is dropped) and the Prewitt gradients under zero padding 1,

        gx_p = (1/3) sum_{dy = -1..1} (t[y + dy][x - 1] - t[y + dy][x + 1]),   gy_p the same on the other axis,
        m_p = sqrt(gx_p^2 + gy_p^2) (no epsilon),   g_p = (2 ma_p mb_p + c) / (ma_p^2 + mb_p^2 + c),

    ``V[n]`` is the population variance of ``g_p`` over the channels and positions of image n: channels are independent grey planes
    pooled inside an image, there is no chroma term."""


def gmsd(a, b, c=0.0026, value_range=(-1., 1.), per_image=False):
    """The gradient magnitude similarity deviation (Xue, Zhang, Mou & Bovik 2014) of two images ``(N, C, H, W)``.
    %s

    ``GMSD[n] = sqrt(V[n])`` on the once-pooled pair ``pool(u_a)``, ``pool(u_b)``; ``c`` defaults to 170 / 255^2.  A distortion: 0 for
    identical images, larger is worse; the value itself is the loss.  The mean over n as a 0-d fp32 tensor, or ``(N,)`` with
    ``per_image``.  Gradients to both images; where ``m_p == 0`` that image's direction ``(gx, gy) / m`` is taken as ``(0, 0)``, and
    where an image's score is 0 its gradient is exactly zero.  Two launches of csrc/gmsd.hip forward and one backward, the pooled
    pair is never stored; under ``no_grad``, or for inputs that need no gradient, nothing is saved, otherwise the two images and a
    (2, 1, N) table.  ``gmsd(x, y) == gmsd(y, x)`` bit for bit with swapped gradients, halving the upstream gradient halves the
    gradients bit for bit, and runs are bit-reproducible.  Every side must be at least 2.  fp32, no double backward."""
    c, lo, hi, _ = _gmsd_check(a, b, c, value_range)
    grad = torch.is_grad_enabled()
    return _GMSD.apply(a.contiguous(), b.contiguous(), None, c, lo, hi, bool(per_image), grad and a.requires_grad, grad and b.requires_grad)


def ms_gmsd(a, b, weights=None, c=0.0026, value_range=(-1., 1.), per_image=False):
    """The multi-scale gradient magnitude similarity deviation (Zhang, Shen, Wang & Li 2017) of two images ``(N, C, H, W)``.
    %s

    ``MS-GMSD[n] = sqrt(sum_j w_j V_j[n])``: scale 1 is the mapped input itself and scale j + 1 is ``pool(scale j)``.  ``weights``
    defaults to (0.096, 0.596, 0.289, 0.019); 1 <= M <= 5 weights, each finite and >= 0, not all zero; a scale of weight 0 contributes
    exactly nothing, so ``ms_gmsd(x, y, weights=(0, 1)) == gmsd(x, y)``.  Every side must be at least ``2^(M - 1)``.  A distortion, 0
    for identical images; the mean over n as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``.  Gradients and singular points as in
    ``gmsd``.  M + 1 launches of csrc/gmsd.hip forward and M backward; saved where an input needs a gradient: the two images, the
    pooled pairs of scales 2..M and a (2, M, N) table.  fp32, no double backward."""
    c, lo, hi, w = _gmsd_check(a, b, c, value_range, MSGMSD_WEIGHTS if weights is None else weights)
    grad = torch.is_grad_enabled()
    return _GMSD.apply(a.contiguous(), b.contiguous(), w, c, lo, hi, bool(per_image), grad and a.requires_grad, grad and b.requires_grad)


if gmsd.__doc__:                                              # python -OO strips docstrings
    gmsd.__doc__ %= _GMSD_DOC
    ms_gmsd.__doc__ %= _GMSD_DOC


# ----------------------------------------------------------------------------------------
# Hessian vesselness and the vessel Dice index (csrc/vessel.hip)
# ----------------------------------------------------------------------------------------
VESSEL_MAX_SCALES = 3
VESSEL_SIGMA_RANGE = (0.5, 3.0)
VESSEL_SIGMAS = (1., 2., 3.)


def _vessel_number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s must be a number, got %r" % (what, v))
    return float(v)


def _vessel_check_scalars(sigmas, weights, beta, c, value_range, eps=0.0):
    """The refusals of ``vesselness`` and ``vessel_dice`` that concern no tensor; returns ``(sigmas, weights, beta, c, eps, lo, hi)`` with
    the scales of weight 0 dropped and the remaining weights normalised to sum 1."""
    beta, c, eps = _vessel_number(beta, "beta"), _vessel_number(c, "c"), _vessel_number(eps, "eps")
    if not (beta > 0 and beta < float("inf")):
        raise ValueError("beta must be positive and finite, got %r" % (beta,))
    if not (c > 0 and c < float("inf")):
        raise ValueError("c must be positive and finite, got %r" % (c,))
    if not (eps >= 0 and eps < float("inf")):
        raise ValueError("eps must be finite and >= 0, got %r" % (eps,))
    try:
        lo, hi = value_range
    except (TypeError, ValueError):
        raise TypeError("value_range must be a pair (lo, hi), got %r" % (value_range,)) from None
    lo, hi = _vessel_number(lo, "value_range's lo"), _vessel_number(hi, "value_range's hi")
    if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite with hi > lo, got %r" % (value_range,))
    try:
        sigmas = tuple(sigmas)
    except TypeError:
        raise TypeError("sigmas must be a sequence of numbers, got %r" % (sigmas,)) from None
    sigmas = tuple(_vessel_number(v, "every sigma") for v in sigmas)
    if not 1 <= len(sigmas) <= VESSEL_MAX_SCALES:
        raise ValueError("sigmas lists 1..%d scales, got %d" % (VESSEL_MAX_SCALES, len(sigmas)))
    if not all(VESSEL_SIGMA_RANGE[0] <= v <= VESSEL_SIGMA_RANGE[1] for v in sigmas):
        raise ValueError("every sigma must lie in [%g, %g], got %r" % (VESSEL_SIGMA_RANGE + (sigmas,)))
    if weights is None:
        weights = (1.0,) * len(sigmas)
    else:
        try:
            weights = tuple(weights)
        except TypeError:
            raise TypeError("weights must be a sequence of numbers, got %r" % (weights,)) from None
        weights = tuple(_vessel_number(v, "every weight") for v in weights)
        if len(weights) != len(sigmas):
            raise ValueError("weights lists one weight per scale, %d of them, got %d" % (len(sigmas), len(weights)))
        if not all(v >= 0 and v < float("inf") for v in weights):
            raise ValueError("every weight must be finite and >= 0, got %r" % (weights,))
        if not any(v > 0 for v in weights):
            raise ValueError("the weights must not all be zero, got %r" % (weights,))
    total = math.fsum(weights)
    kept = [(s, w / total) for s, w in zip(sigmas, weights) if w > 0]
    return tuple(s for s, _ in kept), tuple(w for _, w in kept), beta, c, eps, lo, hi


def _vessel_check_tensors(tensors):
    for t, what in tensors:
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor, got %s" % (what, t.dtype))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    first = tensors[0][0]
    for t, what in tensors[1:]:
        if t.shape != first.shape:
            raise ValueError("%s and %s must have the same shape, got %s and %s" % (tensors[0][1], what, tuple(first.shape), tuple(t.shape)))
    if first.numel() == 0:
        raise ValueError("the filter takes non-empty images, got %s" % (tuple(first.shape),))
    for t, what in tensors:
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    for t, what in tensors[1:]:
        if t.device != first.device:
            raise ValueError("%s and %s must be on one device, got %s and %s" % (tensors[0][1], what, first.device, t.device))


def _vessel_arrays(sigmas, weights):
    M = len(sigmas)
    return (ctypes.cast((ctypes.c_double * M)(*sigmas), ctypes.c_void_p), ctypes.cast((ctypes.c_double * M)(*weights), ctypes.c_void_p), M)


class _Vesselness(Function):
    """``apply(x, cfg, want) -> response map``, ``cfg = (sigmas, weights, beta, c, lo, hi, bright)``.  One ``vessel_index`` in its
    one-image form forward, one ``vessel_grad`` in its map form backward; saved where the input needs a gradient: the image."""

    @staticmethod
    def forward(ctx, x, cfg, want):
        sigmas, weights, beta, c, lo, hi, bright = cfg
        N, C, H, W = x.shape
        out = torch.empty_like(x)
        sg, wt, M = _vessel_arrays(sigmas, weights)
        call("vessel_index", ptr(x), None, ptr(out), None, None, N, C, H, W, sg, wt, M, beta, c, lo, hi, int(bright), stream_ptr())
        ctx.cfg, ctx.want = cfg, want
        if want:
            ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if not ctx.want:
            raise _lib.KernelError("vesselness's forward ran without gradients enabled for this input: nothing was saved")
        sigmas, weights, beta, c, lo, hi, bright = ctx.cfg
        x, = ctx.saved_tensors
        N, C, H, W = x.shape
        g = _c(g)
        dx = torch.empty_like(x)
        sg, wt, M = _vessel_arrays(sigmas, weights)
        call("vessel_grad", ptr(x), None, None, None, None, ptr(g), 0, ptr(dx), None, N, C, H, W, sg, wt, M, beta, c, lo, hi,
             int(bright), stream_ptr())
        return dx, None, None


class _VesselDice(Function):
    """``apply(a, b, cfg, eps, per_image, want_a, want_b) -> score``.  ``vessel_index`` and ``vessel_final`` forward, one ``vessel_grad``
    backward.  Saved where an input needs a gradient: the two images, their two response maps, which ``vessel_index`` then also writes,
    and the (2, N) table; otherwise nothing.  The backward reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, cfg, eps, per_image, want_a, want_b):
        sigmas, weights, beta, c, lo, hi, bright = cfg
        N, C, H, W = a.shape
        dev = a.device
        n = _lib.load().faoctasr_vessel_workspace_floats(N, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_vessel_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "vessel")                 # per stream: consumed by the same call's last launch
        want = want_a or want_b
        ma = torch.empty_like(a) if want else None
        mb = torch.empty_like(b) if want else None
        table = torch.empty((2, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = None if per_image else torch.empty((), dtype=torch.float32, device=dev)
        sg, wt, M = _vessel_arrays(sigmas, weights)
        call("vessel_index", ptr(a), ptr(b), ptr(ma), ptr(mb), ws.data_ptr(), N, C, H, W, sg, wt, M, beta, c, lo, hi, int(bright), stream_ptr())
        call("vessel_final", ws.data_ptr(), N, C, H, W, eps, int(not per_image), ptr(out_image), ptr(out_mean), ptr(table), stream_ptr())
        ctx.cfg = (cfg, want_a, want_b)
        if want:
            ctx.save_for_backward(a, b, ma, mb, table)
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        cfg, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 7
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("vessel_dice's forward ran without gradients enabled for this input: nothing was saved")
        sigmas, weights, beta, c, lo, hi, bright = cfg
        a, b, ma, mb, table = ctx.saved_tensors
        N, C, H, W = a.shape
        g = _c(g).reshape(-1)
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        sg, wt, M = _vessel_arrays(sigmas, weights)
        call("vessel_grad", ptr(a), ptr(b), ptr(ma), ptr(mb), ptr(table), ptr(g), g.numel(), ptr(da), ptr(db), N, C, H, W, sg, wt, M, beta, c,
             lo, hi, int(bright), stream_ptr())
        return (da, db) + (None,) * 5


_VESSEL_DOC = """With ``u = (x - lo) / (hi - lo)`` for ``value_range = (lo, hi)`` and, per scale ``sigma``, ``R = int(3 sigma + 0.5)``, ``t = -R..R``,
    ``g = exp(-t^2 / (2 sigma^2))`` normalised to sum 1, ``g1 = -t / sigma^2 g``, ``g2 = (t^2 / sigma^4 - 1 / sigma^2) g`` (scipy's sampled
    kernels, nothing renormalised), the scale-normalised Hessian under zero padding is

        a = sigma^2 (g2 along W, g along H) * u,   b = sigma^2 (g1, g1) * u,   d = sigma^2 (g along W, g2 along H) * u,

    negated with ``bright=False`` (dark ridges).  ``m = (a + d) / 2``, ``h = (a - d) / 2``, ``r = sqrt(h^2 + b^2)``, ``kappa = r - m`` (minus
    the most negative eigenvalue, the ridge strength), ``mu = m + r``, ``E1 = mu^2 / (2 beta^2 kappa^2)``, ``E2 = (mu^2 + kappa^2) / (2 c^2)`` and

        V = exp(-E1) (1 - exp(-E2)) where kappa > 0 and E1 < 87, exactly 0 with zero gradient elsewhere;   Rsp = sum_s w_s V_s.

    This is Frangi's 2-D measure wherever ``m < 0``; ordering the eigenvalues by value instead of magnitude replaces Frangi's jump to 0
    at ``m >= 0`` by the measure's continuous extension.  The scales are summed with weights, not maximised: the gradient of a maximum
    jumps wherever the arg-max changes.  ``sigmas``: 1 to 3 values in [0.5, 3]; ``weights`` default to equal, each finite and >= 0, not
    all zero, normalised to sum 1; a scale of weight 0 is dropped before anything is launched.  At ``r == 0`` the direction
    ``(h, b) / r`` is taken as ``(0, 0)``.  Channels are independent grey planes; any sides >= 1; fp32, no double backward."""


def vesselness(x, sigmas=VESSEL_SIGMAS, weights=None, beta=0.5, c=0.1, value_range=(-1., 1.), bright=True):
    """The multi-scale Hessian vesselness (Frangi et al. 1998, made continuous) of ``x`` ``(N, C, H, W)``: the response ``Rsp``, the shape of ``x``.
    %s

    One launch of csrc/vessel.hip forward and one backward; saved where ``x`` needs a gradient: ``x``."""
    sigmas, weights, beta, c, _, lo, hi = _vessel_check_scalars(sigmas, weights, beta, c, value_range)
    _vessel_check_tensors([(x, "x")])
    want = torch.is_grad_enabled() and x.requires_grad
    return _Vesselness.apply(x.contiguous(), (sigmas, weights, beta, c, lo, hi, bool(bright)), want)


def vessel_dice(a, b, sigmas=VESSEL_SIGMAS, weights=None, beta=0.5, c=0.1, eps=1e-6, value_range=(-1., 1.), bright=True, per_image=False):
    """The continuous Dice overlap of the vessel maps of two images ``(N, C, H, W)``.
    %s

    ``S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps)`` with ``A = Rsp(a)``, ``B = Rsp(b)`` and the means over the channels and
    positions of image n: ``0 < S <= 1``, 1 for identical images and for two vessel-free images; the loss is ``1 - S``.  The mean over n
    as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``.  Gradients to both images.  Two calls into csrc/vessel.hip forward
    (``vessel_index``, ``vessel_final``) and one backward (``vessel_grad``); under ``no_grad``, or for inputs that need no gradient,
    nothing is saved, otherwise the two images, their two response maps and a (2, N) table.  ``vessel_dice(x, y) == vessel_dice(y, x)``
    bit for bit with swapped gradients, halving the upstream gradient halves the gradients bit for bit, and runs are bit-reproducible."""
    sigmas, weights, beta, c, eps, lo, hi = _vessel_check_scalars(sigmas, weights, beta, c, value_range, eps)
    _vessel_check_tensors([(a, "a"), (b, "b")])
    grad = torch.is_grad_enabled()
    return _VesselDice.apply(a.contiguous(), b.contiguous(), (sigmas, weights, beta, c, lo, hi, bool(bright)), eps, bool(per_image),
                             grad and a.requires_grad, grad and b.requires_grad)


if vesselness.__doc__:                                        # python -OO strips docstrings
    vesselness.__doc__ %= _VESSEL_DOC
    vessel_dice.__doc__ %= _VESSEL_DOC


# ----------------------------------------------------------------------------------------
# Visual information fidelity in the pixel domain (csrc/vif.hip)
# ----------------------------------------------------------------------------------------
VIF_SCALES = 4
VIF_MIN_SIDE = 41
VIF_EPS = 1e-8


def vif_window(scale):
    """The taps of scale ``scale``'s window as Python floats: ``K = 2^(4 - scale) + 1``, ``exp(-(k - (K-1)/2)^2 / (2 (K/5)^2))`` normalised to sum 1."""
    K = (1 << (4 - scale)) + 1
    v = [math.exp(-((k - (K - 1) / 2.0) ** 2) / (2.0 * (K / 5.0) ** 2)) for k in range(K)]
    total = math.fsum(v)
    return [t / total for t in v]


def vif_sides(side):
    """The sides of the four scales' images for a side of scale 0: ``side_{s+1} = (side_s - K_{s+1} + 2) // 2``."""
    out = [int(side)]
    for s in range(1, VIF_SCALES):
        out.append((out[-1] - ((1 << (4 - s)) + 1) + 2) // 2)
    return out


def _vif_check_scalars(sigma_n_sq, value_range):
    """The refusals of ``vif`` that concern no tensor; returns ``(sigma_n_sq, lo, hi)``."""
    sn = _vessel_number(sigma_n_sq, "sigma_n_sq")
    if not (sn > 0 and sn < float("inf")):
        raise ValueError("sigma_n_sq must be positive and finite, got %r" % (sigma_n_sq,))
    try:
        lo, hi = value_range
    except (TypeError, ValueError):
        raise TypeError("value_range must be a pair (lo, hi), got %r" % (value_range,)) from None
    lo, hi = _vessel_number(lo, "value_range's lo"), _vessel_number(hi, "value_range's hi")
    if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite with hi > lo, got %r" % (value_range,))
    return sn, lo, hi


def _vif_check_tensors(a, b):
    for t, what in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor, got %s" % (what, t.dtype))
        if t.dim() != 4:
            raise ValueError("%s must be (N, C, H, W), got %s" % (what, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("vif takes non-empty images, got %s" % (tuple(a.shape),))
    if a.shape[2] < VIF_MIN_SIDE or a.shape[3] < VIF_MIN_SIDE:
        raise ValueError("vif needs sides >= %d (one position of the coarsest scale sees %d x %d pixels), got %s"
                         % (VIF_MIN_SIDE, VIF_MIN_SIDE, VIF_MIN_SIDE, tuple(a.shape)))
    for t, what in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise ValueError("%s must be on a GPU device, got %s" % (what, t.device))
    if a.device != b.device:
        raise ValueError("a and b must be on one device, got %s and %s" % (a.device, b.device))


class _VIF(Function):
    """``apply(a, b, sigma_n_sq, lo, hi, per_image, want_a, want_b) -> score``.  Four ``vif_scale_fwd`` and one ``vif_final`` forward, four
    ``vif_scale_bwd`` backward, coarsest first.  Saved where an input needs a gradient: the two images, the pairs of scales 1..3, which
    the forward writes in any case, and the (2, N) table; otherwise nothing.  The backward reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, a, b, sn, lo, hi, per_image, want_a, want_b):
        N, C, H, W = a.shape
        dev = a.device
        n = _lib.load().faoctasr_vif_workspace_floats(N, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_vif_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "vif")                    # per stream: consumed by the same call's last launch
        want = want_a or want_b
        hs, wsd = vif_sides(H), vif_sides(W)
        xs, rs = [a], [b]
        for s in range(1, VIF_SCALES):
            xs.append(torch.empty((N, C, hs[s], wsd[s]), dtype=torch.float32, device=dev))
            rs.append(torch.empty((N, C, hs[s], wsd[s]), dtype=torch.float32, device=dev))
        table = torch.empty((2, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = None if per_image else torch.empty((), dtype=torch.float32, device=dev)
        for s in range(VIF_SCALES):
            last = s == VIF_SCALES - 1
            call("vif_scale_fwd", ptr(xs[s]), ptr(rs[s]), None if last else ptr(xs[s + 1]), None if last else ptr(rs[s + 1]), ws.data_ptr(),
                 N, C, H, W, s, lo, hi, sn, stream_ptr())
        call("vif_final", ws.data_ptr(), N, C, H, W, int(not per_image), ptr(out_image), ptr(out_mean), ptr(table), stream_ptr())
        ctx.cfg = (sn, lo, hi, want_a, want_b)
        if want:
            ctx.save_for_backward(*(xs + rs + [table]))
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        sn, lo, hi, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 8
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("vif's forward ran without gradients enabled for this input: nothing was saved")
        saved = ctx.saved_tensors
        xs, rs, table = saved[:VIF_SCALES], saved[VIF_SCALES:2 * VIF_SCALES], saved[2 * VIF_SCALES]
        N, C, H, W = xs[0].shape
        g = _c(g).reshape(-1)
        da = db = None
        for s in reversed(range(VIF_SCALES)):
            na = torch.empty_like(xs[s]) if need_a else None
            nb = torch.empty_like(rs[s]) if need_b else None
            call("vif_scale_bwd", ptr(xs[s]), ptr(rs[s]), ptr(table), ptr(g), g.numel(), ptr(da), ptr(db), ptr(na), ptr(nb), N, C, H, W, s,
                 lo, hi, sn, stream_ptr())
            da, db = na, nb
        return (da, db) + (None,) * 6


def vif(a, b, sigma_n_sq=2.0, value_range=(-1., 1.), per_image=False):
    """The visual information fidelity in the pixel domain (VIFp; Sheikh & Bovik 2006) of ``a``, the image under test, against ``b``, the
    reference, both ``(N, C, H, W)`` with ``H, W >= 41``: the Gaussian-channel information ``a`` keeps about ``b`` over the information
    ``b`` itself carries, against a visual-noise floor ``sigma_n_sq``, at four scales.

    With ``u = (t - lo) * 255 / (hi - lo)`` for ``value_range = (lo, hi)``, ``EPS = 1e-8`` and, per scale ``s = 0..3``, the window ``w_s`` of
    ``K_s = 2^(4-s) + 1`` taps ``exp(-(k - (K_s-1)/2)^2 / (2 (K_s/5)^2))`` normalised to sum 1 and ``W_s * t`` its separable VALID convolution:
    at ``s > 0`` both images are first filtered with the new scale's window and decimated (``[::2, ::2]``); then ``mx = W_s*x``, ``mr = W_s*r``,
    ``sxx = relu(W_s*(x x) - mx^2)``, ``srr = relu(W_s*(r r) - mr^2)``, ``sxr = W_s*(x r) - mx mr``, ``g = sxr / (srr + EPS)``, ``sv = sxx - g sxr``,
    and in this order: where ``srr < EPS``: ``g = 0, sv = sxx, srr = 0``; where ``sxx < EPS``: ``g = 0, sv = 0``; where ``g < 0``: ``sv = sxx, g = 0``;
    where ``sv <= EPS``: ``sv = EPS``.

        V[n] = (sum_s sum log10(1 + g^2 srr / (sv + sigma_n_sq)) + EPS) / (sum_s sum log10(1 + srr / sigma_n_sq) + EPS)

    with the inner sums over the channels and positions of image n.  ``V(a, b)`` is NOT ``V(b, a)``: a reconstruction that adds contrast the
    reference lacks can score above 1, a blurred one scores below 1, and regions whose local contrast sits below the noise floor cost
    almost nothing.  ``V(t, t)`` is 1 up to rounding; the loss is ``1 - V``.  The mean over n as a 0-d fp32 tensor, or ``(N,)`` with
    ``per_image``.  Gradients to both images; a ``where`` passes the gradient of the branch it took, ``relu'(0) = 0``, a clamped value
    passes none.  Channels are independent grey planes; fp32, no double backward.

    Five calls into csrc/vif.hip forward (four ``vif_scale_fwd``, ``vif_final``) and four backward (``vif_scale_bwd``, coarsest first);
    under ``no_grad``, or for inputs that need no gradient, nothing is saved, otherwise the two images, the pairs of scales 1..3 (a third
    of the inputs) and a (2, N) table.  Halving the upstream gradient halves the gradients bit for bit, one side's gradient has the
    same bits with or without the other's, and runs are bit-reproducible."""
    sn, lo, hi = _vif_check_scalars(sigma_n_sq, value_range)
    _vif_check_tensors(a, b)
    grad = torch.is_grad_enabled()
    return _VIF.apply(a.contiguous(), b.contiguous(), sn, lo, hi, bool(per_image), grad and a.requires_grad, grad and b.requires_grad)


# ----------------------------------------------------------------------------------------
# Soft skeletons and soft-clDice (csrc/cldice.hip)
# ----------------------------------------------------------------------------------------
CLDICE_MAX_ITERS = 10


def _cldice_check_scalars(iters, value_range, smooth=0.0):
    """The refusals of ``soft_skeleton`` and ``cldice`` that concern no tensor; returns ``(iters, smooth, lo, hi)``."""
    if isinstance(iters, bool) or not isinstance(iters, int):
        raise TypeError("iters must be an integer, got %r" % (iters,))
    if not 1 <= iters <= CLDICE_MAX_ITERS:
        raise ValueError("iters must lie in 1..%d (the halo of iters + 2 is staged in LDS), got %d" % (CLDICE_MAX_ITERS, iters))
    smooth = _vessel_number(smooth, "smooth")
    if not (smooth >= 0 and smooth < float("inf")):
        raise ValueError("smooth must be finite and >= 0, got %r" % (smooth,))
    try:
        lo, hi = value_range
    except (TypeError, ValueError):
        raise TypeError("value_range must be a pair (lo, hi), got %r" % (value_range,)) from None
    lo, hi = _vessel_number(lo, "value_range's lo"), _vessel_number(hi, "value_range's hi")
    if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("value_range must be finite with hi > lo, got %r" % (value_range,))
    return iters, smooth, lo, hi


def _cldice_records(like, iters):
    """The records of one image: ``iters + 1`` coefficient maps and as many maps of selection bytes, 5 (iters + 1) bytes per sample."""
    return (torch.empty((iters + 1,) + tuple(like.shape), dtype=torch.float32, device=like.device),
            torch.empty((iters + 1,) + tuple(like.shape), dtype=torch.uint8, device=like.device))


class _SoftSkeleton(Function):
    """``apply(x, iters, lo, hi, bright, want) -> skeleton map``.  One ``cldice_index`` in its one-image form forward, one ``cldice_grad``
    in its map form backward; saved where the input needs a gradient: its records (``_cldice_records``), not the image."""

    @staticmethod
    def forward(ctx, x, iters, lo, hi, bright, want):
        N, C, H, W = x.shape
        out = torch.empty_like(x)
        rec, sel = _cldice_records(x, iters) if want else (None, None)
        call("cldice_index", ptr(x), None, ptr(out), None, ptr(rec), None if sel is None else sel.data_ptr(), None, None, None, N, C, H, W, iters,
             lo, hi, int(bright), stream_ptr())
        ctx.cfg = (iters, lo, hi, bright, want)
        if want:
            ctx.save_for_backward(rec, sel)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        iters, lo, hi, bright, want = ctx.cfg
        if not want:
            raise _lib.KernelError("soft_skeleton's forward ran without gradients enabled for this input: nothing was saved")
        rec, sel = ctx.saved_tensors
        _, N, C, H, W = rec.shape
        g = _c(g)
        dx = torch.empty_like(g)
        call("cldice_grad", None, None, ptr(rec), sel.data_ptr(), None, None, None, None, None, ptr(g), 0, ptr(dx), None, N, C, H, W, iters, lo, hi,
             int(bright), stream_ptr())
        return (dx,) + (None,) * 5


class _ClDice(Function):
    """``apply(a, b, iters, smooth, lo, hi, bright, per_image, want_a, want_b) -> score``.  ``cldice_index`` and ``cldice_final`` forward, one
    ``cldice_grad`` backward.  Saved per input that needs a gradient: its records and the other image's skeleton map, which ``cldice_index``
    then also writes, besides the two images and the (4, N) table; otherwise nothing.  The backward reads the upstream gradient on the
    device."""

    @staticmethod
    def forward(ctx, a, b, iters, smooth, lo, hi, bright, per_image, want_a, want_b):
        N, C, H, W = a.shape
        dev = a.device
        n = _lib.load().faoctasr_cldice_workspace_floats(N, C, H, W)
        if n < 0:
            raise _lib.KernelError("faoctasr_cldice_workspace_floats failed: %s" % _lib.load().faoctasr_last_error().decode())
        ws = _lib.workspace(dev, n, "cldice")                 # per stream: consumed by the same call's last launch
        want = want_a or want_b
        rec_a, sel_a = _cldice_records(a, iters) if want_a else (None, None)
        rec_b, sel_b = _cldice_records(b, iters) if want_b else (None, None)
        skel_a = torch.empty_like(a) if want_b else None
        skel_b = torch.empty_like(b) if want_a else None
        table = torch.empty((4, N), dtype=torch.float32, device=dev) if want else None
        out_image = torch.empty((N,), dtype=torch.float32, device=dev)
        out_mean = None if per_image else torch.empty((), dtype=torch.float32, device=dev)
        call("cldice_index", ptr(a), ptr(b), ptr(skel_a), ptr(skel_b), ptr(rec_a), None if sel_a is None else sel_a.data_ptr(), ptr(rec_b),
             None if sel_b is None else sel_b.data_ptr(), ws.data_ptr(), N, C, H, W, iters, lo, hi, int(bright), stream_ptr())
        call("cldice_final", ws.data_ptr(), N, C, H, W, smooth, int(not per_image), ptr(out_image), ptr(out_mean), ptr(table), stream_ptr())
        ctx.cfg = (iters, lo, hi, bright, want_a, want_b)
        if want:
            ctx.save_for_backward(*[t for t in (a, b, table, rec_a, sel_a, skel_b, rec_b, sel_b, skel_a) if t is not None])
        return out_image if per_image else out_mean

    @staticmethod
    def backward(ctx, g):
        iters, lo, hi, bright, want_a, want_b = ctx.cfg
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 10
        if (need_a and not want_a) or (need_b and not want_b):
            raise _lib.KernelError("cldice's forward ran without gradients enabled for this input: nothing was saved")
        saved = list(ctx.saved_tensors)
        a, b, table = saved[:3]
        rest = saved[3:]
        rec_a, sel_a, skel_b = rest[:3] if want_a else (None, None, None)
        rec_b, sel_b, skel_a = rest[3 if want_a else 0:][:3] if want_b else (None, None, None)
        N, C, H, W = a.shape
        g = _c(g).reshape(-1)
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        call("cldice_grad", ptr(a), ptr(b), ptr(rec_a), None if sel_a is None else sel_a.data_ptr(), ptr(rec_b),
             None if sel_b is None else sel_b.data_ptr(), ptr(skel_a), ptr(skel_b), ptr(table), ptr(g), g.numel(), ptr(da), ptr(db), N, C, H, W,
             iters, lo, hi, int(bright), stream_ptr())
        return (da, db) + (None,) * 8


_CLDICE_DOC = """With ``u = (x - lo) / (hi - lo)`` for ``value_range = (lo, hi)`` (``(hi - x) / (hi - lo)`` with ``bright=False``: dark vessels), ``E(I)[q]`` the
    minimum of ``I`` over the 5-point cross around ``q`` and ``D(I)[q]`` the maximum over the 3 x 3 square, positions outside the image left out
    (``max_pool2d`` with its implicit padding), and ``K = iters``:

        I_0 = u,  I_{k+1} = E(I_k),  O_k = D(I_{k+1}),  delta_k = relu(I_k - O_k),  k = 0..K
        s_0 = delta_0,  s_k = s_{k-1} + relu(delta_k - s_{k-1} delta_k),  skel(u) = s_K

    the soft skeleton of Shit et al. (CVPR 2021).  ``iters`` is an integer in 1..10 (the authors' default is 3; for retinal vessels they
    go up to the largest vessel radius in pixels; the limit is the halo of ``iters + 2`` the kernels keep in LDS).  ``relu'(0) = 0``.
    Ties: the result does not depend on which of several equal values a minimum or maximum takes; the gradient sends the whole
    cotangent to the FIRST of the tied positions in row-major order (cross: up, left, centre, right, down; square: top-left to
    bottom-right).  That is a valid subgradient and conserves the total; where the values of a plane are distinct it is the gradient,
    and on plateaus (a quantised image, the exact zeros of a vesselness map) it differs from ``max_pool2d``'s backward, whose choice
    depends on its scan order.  Channels are independent grey planes; any sides >= 1; finite inputs; fp32, no double backward."""


def soft_skeleton(x, iters=3, value_range=(-1., 1.), bright=True):
    """The soft skeleton of ``x`` ``(N, C, H, W)`` by iterated min / max pooling: a map the shape of ``x``, differentiable.
    %s

    One launch of csrc/cldice.hip forward and one backward; saved where ``x`` needs a gradient: 5 (iters + 1) bytes per sample (per level
    one coefficient and one selection byte), by which the backward routes an arbitrary upstream map."""
    iters, _, lo, hi = _cldice_check_scalars(iters, value_range)
    _vessel_check_tensors([(x, "x")])
    want = torch.is_grad_enabled() and x.requires_grad
    return _SoftSkeleton.apply(x.contiguous(), iters, lo, hi, bool(bright), want)


def cldice(a, b, iters=3, smooth=1.0, value_range=(-1., 1.), bright=True, per_image=False):
    """Soft-clDice, the centre-line Dice of two images ``(N, C, H, W)``: how much of each image's soft skeleton lies inside the other image.
    %s

    Per image n, the sums over its channels and positions:

        Tprec = (sum skel(a) u_b + smooth) / (sum skel(a) + smooth),   Tsens = (sum skel(b) u_a + smooth) / (sum skel(b) + smooth)
        S[n] = 2 Tprec Tsens / (Tprec + Tsens), 0 where that denominator is 0; a ratio whose own denominator is 0 is taken as 0

    ``smooth >= 0`` acts on sums, not means, as in the authors' code; unlike theirs the sums run per image and the batch is averaged, as
    every index here does.  The loss is ``1 - S``.  The mean over n as a 0-d fp32 tensor, or ``(N,)`` with ``per_image``.  Gradients to
    both images.  Two calls into csrc/cldice.hip forward (``cldice_index``, ``cldice_final``) and one backward (``cldice_grad``); under
    ``no_grad``, or for inputs that need no gradient, nothing is saved, otherwise the two images, a (4, N) table and per input that
    needs a gradient its 5 (iters + 1) bytes per sample of records and the other image's skeleton map.  ``cldice(x, y) == cldice(y, x)``
    bit for bit with swapped gradients, halving the upstream gradient halves the gradients bit for bit, one side's gradient has the
    same bits with or without the other's, and runs are bit-reproducible.  On vessel maps: ``cldice(vesselness(x), vesselness(y),
    value_range=(0, 1))`` composes through autograd; such maps hold regions of exactly 0, plateaus on which the tie rule above applies."""
    iters, smooth, lo, hi = _cldice_check_scalars(iters, value_range, smooth)
    _vessel_check_tensors([(a, "a"), (b, "b")])
    grad = torch.is_grad_enabled()
    return _ClDice.apply(a.contiguous(), b.contiguous(), iters, smooth, lo, hi, bool(bright), bool(per_image), grad and a.requires_grad,
                         grad and b.requires_grad)


if soft_skeleton.__doc__:                                     # python -OO strips docstrings
    soft_skeleton.__doc__ %= _CLDICE_DOC
    cldice.__doc__ %= _CLDICE_DOC
