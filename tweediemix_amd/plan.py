"""The launch recorder every network of this package is built on (UNet, video UNet, VAE decoder / encoder).

A plan is a fixed list of (C entry point, argument tuple), recorded once and replayed -- eagerly or inside a captured graph -- by a
loop that allocates nothing.  This module holds what all plans share and nothing about any one network: the buffer arena, the op
list, the bookkeeping bench.py and the tuner read (flops, launches, op_meta, _tunable) and the weight-prefetch hints.  Host code only.

Two kinds of op exist.  `_emit` records a launch the library does not stamp under tmix_prof_begin (embeddings, conv_in / conv_out,
concat, quantiser, softmax, ...).  `_launch` records one it does stamp -- by name, the entry points of STAMPED -- and is the single place that
appends to `launches` / `_tunable`, writes `op_meta` and patches the previous launch's hint slot.  `_freeze`, called at the end of
every `_build`, checks that the two were not mixed up: the profiler deals its slots out in issue order, so one stamped launch
without an op_meta entry would shift every later stamp.
"""
from __future__ import annotations

import os

import torch

from . import lib as L

BF16 = torch.bfloat16

# entry point -> class of its op_meta entry: exactly the launches that take a profiler slot (csrc: tmix_prof_take)
STAMPED = {
    "tmix_gemm_bf16": "gemm", "tmix_gemm_q_cross_attn": "gemm",
    "tmix_gemm_fp8": "gemm_fp8",                                    # its own class: priced against the fp8 MFMA peak (bench.py)
    "tmix_conv3x3_nhwc": "conv", "tmix_conv3x3_nhwc_fp8": "conv_fp8",
    "tmix_groupnorm_nhwc": "norm", "tmix_groupnorm_nhwc_pre": "norm", "tmix_groupnorm_nhwc_pre_f8": "norm",
    "tmix_attn_fwd_ws": "attn", "tmix_attn_fwd_f8_ws": "attn",
}
_FAMILY = {"gemm": "gemm", "gemm_fp8": "gemm", "conv": "conv", "conv_fp8": "conv", "attn": "attn"}      # class -> key of `launches` (norms: none)


def hint_bytes(nbytes, cap, over):
    """bytes of an `nbytes` weight tensor that the launch in front of its consumer touches (tmix_gemm_prefetch_next):
    tensors larger than `over` are named by their first `cap` bytes (cap 0: whole tensors)"""
    return min(nbytes, cap) if cap and nbytes > over else nbytes


class ParamRing:
    """Pinned staging ring for a step's eight parameter floats (image and video sampler; width=12 for the image sampler's stochastic steps).  The host
    runs ahead of the device by whole steps: next() hands out a slot once the copy that last read it has completed, upload(dst) copies it
    asynchronously and records (n: only the slot's first n floats into dst's first n).  cuda=False: pageable, no events."""

    def __init__(self, cuda=True, slots=64, width=8):
        z = torch.zeros(slots, width, dtype=torch.float32)
        self.slots, self.events, self.i, self.cuda = (z.pin_memory() if cuda else z), [None] * slots, -1, cuda

    def next(self):
        self.i = (self.i + 1) % len(self.events)
        if self.events[self.i] is not None:
            self.events[self.i].synchronize()
        return self.slots[self.i]

    def upload(self, dst, n=None):
        if n is None:
            dst.copy_(self.slots[self.i], non_blocking=True)
        else:
            dst[:n].copy_(self.slots[self.i][:n], non_blocking=True)
        if self.cuda:
            self.events[self.i] = torch.cuda.Event()
            self.events[self.i].record()


class Arena:
    """Size-keyed free list: the plan is a static, stream-ordered launch sequence, so a buffer released
    at plan position i can be handed to any op planned after i."""

    def __init__(self, device):
        self.device, self.free, self.total = device, {}, 0
        self.bufs = []          # owns every buffer for the plan's lifetime (views handed out are not owners)

    def get(self, *shape, dtype=BF16):
        n = 1
        for s in shape:
            n *= s
        nbytes = (n * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
        lst = self.free.get(nbytes)
        if lst:
            buf = lst.pop()
        else:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.bufs.append(buf)
            self.total += nbytes
        tns = buf.view(dtype)[:n].view(*shape)
        tns._arena_buf = buf
        return tns

    def put(self, *ts):
        for tns in ts:
            buf = tns._arena_buf
            self.free.setdefault(buf.numel(), []).append(buf)
            for cs, _c in getattr(tns, "_cs", None) or ():  # GroupNorm column partials of this tensor (the plans' _colstats): every reader came before
                self.put(cs)
            tns._cs = None


class LaunchPlan:
    """What every plan records into and replays from.

    ops         [(fn, args)] in issue order; fn.__name__ is the entry point, the stream is appended when the op runs
    keep        descriptors / tensors that must outlive the plan
    flops, gemm_flops, launches["gemm" | "conv" | "attn"] = [(descriptor or args, flops)]
    op_meta     index into ops -> (class, flops, key) of the stamped launches; issued_meta() lists them in issue order
    _tunable    [(index into ops, kind, descriptor)] of the launches whose tiling the tuner may change

    hints = (cap, over) bytes, see hint_bytes.  TMIX_NO_PREFETCH=1 records no hints at all."""

    def __init__(self, device, hints=(0, 0), lib=None):
        self.lib = L.load() if lib is None else lib
        self.dev = device
        self.ops = []
        self.keep = []
        self.arena = Arena(device)
        self.flops = 0
        self.gemm_flops = 0
        self.launches = {"gemm": [], "conv": [], "attn": []}
        self.op_meta = {}
        self._tunable = []
        # a hinted launch is preceded by a tmix_gemm_prefetch_next op naming the weights of the hinted launch AFTER it (patched in
        # when that launch is recorded): the chain otherwise meets every weight cold from HBM
        self._pf_on = not os.environ.get("TMIX_NO_PREFETCH")
        self._pf_cap, self._pf_cap_over = hints
        self._pf_prev = None

    def _emit(self, fn, *args):
        """record a launch the library does not stamp"""
        self.ops.append((fn, args))

    def _launch(self, name, args, flops, key=None, gemm_flops=0, desc=None, weight=None, tunable=None, keep=()):
        """record one stamped launch lib.<name>(*args, stream).  flops: all of it, gemm_flops: the part that counts as GEMM flops;
        key: third field of its op_meta entry (default: the descriptor); desc: its descriptor, kept alive and listed in `launches`
        (without one the args are listed); weight: the tensor the previous hinted launch is to prefetch -- None records no hint;
        tunable: "gemm" / "conv" when the tuner may re-tile `desc`; keep: whatever else the args point into."""
        cls, fn = STAMPED[name], getattr(self.lib, name)
        self.keep += [o for o in (desc, *keep) if o is not None]
        if weight is not None and self._pf_on:
            if self._pf_prev is not None:
                self._pf_prev[0], self._pf_prev[1] = weight.data_ptr(), hint_bytes(weight.numel() * weight.element_size(), self._pf_cap, self._pf_cap_over)
            self._pf_prev = [None, 0]
            self.keep.append(weight)
            self.ops.append((self.lib.tmix_gemm_prefetch_next, self._pf_prev))
        i = len(self.ops)
        self.ops.append((fn, args))
        self.flops += flops
        self.gemm_flops += gemm_flops
        if cls in _FAMILY:      # (a GEMM launch is listed with its GEMM flops: tmix_gemm_q_cross_attn's attention half is not the tuner's)
            self.launches[_FAMILY[cls]].append((desc if desc is not None else args, gemm_flops if _FAMILY[cls] == "gemm" else flops))
        if tunable is not None:
            self._tunable.append((i, tunable, desc))
        self.op_meta[i] = (cls, flops, desc if key is None else key)

    def _freeze(self):
        """end of recording: args become tuples (the hint slots were lists until patched), and the profiler-slot invariant is checked"""
        for i, (fn, _a) in enumerate(self.ops):
            name = getattr(fn, "__name__", "")      # (a test that wraps the library's functions leaves other names: nothing to tell then)
            ok = (name in STAMPED or not name.startswith("tmix_")) if i in self.op_meta else name not in STAMPED
            assert ok, f"op {i} ({name}): stamped launches are recorded by _launch, all others by _emit"
        self.ops = [(fn, tuple(a)) for fn, a in self.ops]

    def issued_meta(self):
        """(class, flops, key) of the instrumented launches (tmix_prof_begin) in the order run() issues them."""
        return [self.op_meta[i] for i in range(len(self.ops)) if i in self.op_meta]

    def run(self, stream=None):
        """enqueue the whole forward on `stream` (default: torch's current stream). No sync, no alloc."""
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        for fn, args in self.ops:
            rc = fn(*args, st)
            if rc:
                L.check(rc, fn.__name__)
