"""torch.autograd.Function wrappers around the C-ABI kernels (host plumbing only).

Conventions used by every layer op
----------------------------------
* layers emit PRE-activations; the consumer applies the activation while it stages its input
  (`in_act`), and its data-gradient kernel multiplies by act'(input) in the epilogue.  No standalone
  activation kernels exist and no layer depends on a neighbour's saved tensors.
* weight/bias gradients: when the caller passes the parameter's preset `.grad` view (`gw`, `gb`; a slice of
  the flat gradient buffer, see flat.py) the kernels ACCUMULATE into it and autograd gets None for that
  input -- no AccumulateGrad kernels, no copies.  Without it, fresh tensors are returned to autograd.
"""
import bisect
import ctypes
import itertools
import math
import os

import numpy as np
import torch
from torch.autograd import Function

from . import hipops as H

_DACT = {H.ACT_NONE: H.EP_NONE, H.ACT_SILU: H.EP_MUL_SILU_GRAD, H.ACT_RELU: H.EP_MUL_RELU_MASK,
         H.ACT_GELU: H.EP_MUL_GELU_GRAD}


CALLS = [0]      # C-ABI calls issued so far (trainer.capture reports how many one captured step holds)


def _call(name, *args):
    CALLS[0] += 1
    H.check(getattr(H.lib(), name)(*args), name)


class GradReducer:
    """Deferred reduction of split weight-gradient partials (one launch per backward instead of ~40).

    While a backward pass runs, every op whose gradient kernel produces split partials takes a PRIVATE slice of
    the step arena for them and registers a segment (partials -> destination in the flat gradient buffer).  An
    autograd-engine callback queued by the first registration fires when the backward pass is complete and folds
    all segments with mmvae_reduce_segments.  Works unchanged under hipGraph capture (fixed arena offsets)."""

    enabled = True
    tail = None       # lincomb_rows_args(...) of an ELBO assembly that rides on the next fold (see flush)
    # defer_next: the caller promises that an optimiser step over the flat buffers follows the backward pass at once
    # (trainer.capture with the optimiser inside the graph).  flush() then only joins the streams and parks the segment
    # table in `deferred`; FlatAdam.step() takes it and folds + updates in ONE launch (mmvae_adam_fold_flat).
    defer_next = False
    deferred = None
    # pre_join(device, side_streams): called at the end of the backward pass right BEFORE the side streams are joined --
    # the place where a tower's stream has finished its gradient work and idles until the optimiser (trainer.capture
    # queues the next batch's host-to-device pull there: MultimodalVAE.capture(..., input_ring=...))
    pre_join = None
    # side_tail: the same work queued EARLIER when the side tower announces its last backward launch (EmbedPE.backward
    # calls run_side_tail): hipGraph submits nodes in capture order, so a node captured at the very end of the backward
    # pass is submitted -- and starts -- late however long its stream has been idle (measured: the pull queued at the
    # join started ~30 us after the text stream went idle and delayed the optimiser by as much)
    side_tail = None
    side_head = None      # fn(device): see StreamIdlePoint
    _arena = {}
    _state = {}

    @classmethod
    def _st(cls, device):
        key = H.device_key(device)
        st = cls._state.get(key)
        if st is None:
            st = {"off": 0, "segs": [], "armed": False, "device": device, "keep": [], "used": set(), "spill": [],
                  "spilled": 0}
            cls._state[key] = st
        return key, st

    @classmethod
    def begin_step(cls, device):
        """start of an objective(): the previous backward pass must have folded and cleared everything.  If it raised
        (autograd skips the final callbacks then) the state is stale -- `armed` would stay set, no later backward
        would queue a fold and the deferred weight gradients would never reach the flat buffer: reset it."""
        if device.type != "cuda":
            return
        _, st = cls._st(device)
        cls.early_step, cls.dw_jobs, cls.dw_open = None, [], False      # (per-step state: a backward pass that raised leaves them behind)
        cls.tw_jobs, cls.early_ready = {}, False
        cls.cw_jobs, cls.cw_done, cls.cw_streams = [], None, None
        cls.last_writer.clear()
        cls.packed_grads.clear()
        cls.packed_uses.clear()
        if cls.deferred is not None:
            cls.deferred = None
            raise RuntimeError("GradReducer: a deferred fold was never taken by an optimiser step: the split weight "
                               "gradients of the previous backward pass were lost")
        if st["armed"] or st["segs"]:
            st.update(off=0, segs=[], armed=False, keep=[], used=set(), spill=[], spilled=0)
            cls.tail = None

    @classmethod
    def alloc(cls, n_floats, device):
        """a private slice of the step arena.  The arena never moves or gets folded in the middle of a backward pass
        (kernels on several streams are writing into it): when it is full a further chunk is chained for the rest of
        the step, and the next step starts with one arena of the combined size."""
        key, st = cls._st(device)
        n = (int(n_floats) + 63) // 64 * 64
        ar = cls._arena.get(key)
        if ar is None or st["off"] + n > ar.numel():
            if ar is not None:
                st["spill"].append(ar)          # keep the full chunk alive until the end-of-backward fold
                st["spilled"] += ar.numel()
            ar = torch.empty(max(n, 16 << 20), dtype=torch.float32, device=device)   # 64 MB chunks
            cls._arena[key] = ar
            st["off"] = 0
            # The caching allocator may hand out memory that kernels already QUEUED on the allocating stream still use
            # (freed on the host, ordered on that stream only) -- but the arena is written from every stream of the step:
            # the other streams wait for what the allocating stream has queued so far.  (Found as a wrong embedding
            # gradient when a large two-stream step followed small ones in one process; only on this first-use / spill
            # path -- the next step starts with an arena allocated at the end-of-backward join.)
            if device.type == "cuda" and StreamPlan.enabled:
                cur = torch.cuda.current_stream(device)
                for other in set(StreamPlan.pair.get(key, ())) | set(st["used"]):
                    if other != cur:
                        other.wait_stream(cur)
        out = ar[st["off"]:st["off"] + n]
        st["off"] += n
        return out

    @classmethod
    def add(cls, src_ptr, dst, rows, length, stride):
        _, st = cls._st(dst.device)
        st["segs"].append((src_ptr, dst.data_ptr(), int(rows), int(length), int(stride)))
        if not st["armed"]:
            st["armed"] = True
            dev = dst.device
            torch.autograd.Variable._execution_engine.queue_callback(lambda: cls.flush(dev))

    @classmethod
    def _merged(cls, segs):
        """Fewer table entries for the same fold.  A segment that CONTINUES the one registered before it -- its source columns
        follow in the same partial rows, its destination follows in the flat gradient: LayerNorm's gamma | beta, the
        feed-forward block's w1 | b1 | w2 | b2, a fused text layer's three LayerNorm pairs -- is the same sum with a longer
        row.  Two ops may reach one parameter through runs of different length (PoE's text decoder: the fused layer registers
        its six LayerNorm tensors as one run, the launch-per-op form of the same layer as three pairs), and the fold needs
        destination ranges that are EQUAL (chained) or DISJOINT: every run is therefore cut at each other run's end points
        (which are boundaries of its own pieces, since the registered pieces are equal-or-disjoint themselves).  Per element
        the same sum in the same order: bit-identical training (test_merged_fold_segments_train_bit_identically).
        cfg1: 67 -> 51 entries (<= 64: the step closes with the ONE fold + Adam launch); cfg5: 213 -> 133, 61 of them in the
        decoders' range (the early optimiser launch takes <= 64)."""
        if not cls.merge_adjacent or len(segs) < 2:
            return list(segs)
        runs = []      # [src, dst, rows, stride, [piece lengths]]
        for sp, dp, r, ln, sd in segs:
            if runs:
                q = runs[-1]
                tot = sum(q[4])
                if sp == q[0] + 4 * tot and dp == q[1] + 4 * tot and r == q[2] and sd == q[3]:
                    q[4].append(ln)
                    continue
            runs.append([sp, dp, r, sd, [ln]])
        ends = sorted({e for q in runs for e in (q[1], q[1] + 4 * sum(q[4]))})
        out = []
        for sp, dp, r, sd, lens in runs:
            end = dp + 4 * sum(lens)
            need = [c for c in ends[bisect.bisect_right(ends, dp):bisect.bisect_left(ends, end)]]
            offs, o = [], 0
            for ln in lens:
                offs.append(o)
                o += ln
            bounds = {dp + 4 * o_ for o_ in offs}
            if any(c not in bounds for c in need):      # (cannot happen for equal-or-disjoint pieces: keep them as registered)
                out.extend((sp + 4 * o_, dp + 4 * o_, r, ln, sd) for o_, ln in zip(offs, lens))
                continue
            cuts = sorted({dp, *need})
            for a, b in zip(cuts, cuts[1:] + [end]):
                out.append((sp + (a - dp), a, r, (b - a) // 4, sd))
        return out

    @staticmethod
    def _check_disjoint(segs):
        """destination ranges of one fold are equal (chained) or disjoint: a partial overlap would be two workgroups adding
        into the same elements (the fused fold + Adam launch refuses it; the plain fold launches would race)"""
        spans = sorted({(dp, dp + 4 * ln) for _, dp, _, ln, _ in segs})
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            if b0 < a1:
                raise RuntimeError(f"GradReducer: fold segments overlap partially: [{a0:#x}, {a1:#x}) and [{b0:#x}, {b1:#x})")

    @staticmethod
    def _table(segs):
        t = H.ReduceSegments()
        for j, (sp, dp, r, ln, sd) in enumerate(segs):
            t.src[j], t.dst[j], t.rows[j], t.len[j], t.stride[j] = sp, dp, r, ln, sd
        t.n = len(segs)
        return t

    @classmethod
    def run_side_tail(cls, device):
        fn, cls.side_tail = cls.side_tail, None
        if fn is not None:
            fn(device, [])                      # on the CURRENT stream = the side tower's

    # early_step = (fn, stream, lo, hi): set by MoPOE.objective_backward for a captured one-GPU step (MMVAE_EARLY_ADAM=2,
    # the default; 0: trainer.capture never arms it).  Once the fusion's backward has been queued on `stream` and handed its
    # gradients over (EarlyStepPoint.backward sets `early_ready`), every gradient of the flat buffer's second range [lo, hi)
    # (decoders, prior: FlatParams.split) is final AND stream-ordered on `stream`, so their fold + Adam update runs beside
    # the encoders' backward instead of in the serial launch at the end of the step: run_early_step, called by _txt_wgrad
    # in front of the weight-gradient launch of the text encoder's layer (fn(table of the range's segments or None)).  The
    # range's segments leave the list: nobody else folds them.  (The other placements that were measured: DESIGN.md 0.)
    early_step = None
    early_ready = False
    # data_ptr of a head output -> [its ONE gradient tensor of this backward pass, fusion calls whose backward is still to
    # come]; packed_uses: how many column-range fusion calls read it in this step's forward pass (PoeReparamKL)
    packed_grads, packed_uses = {}, {}
    share_packed_grads = True     # (module switch for the tests)

    @classmethod
    def packed_grads_done(cls):
        """end of a backward pass: every shared gradient tensor must have been handed over by its last reader"""
        left = [k for k, (_, n) in cls.packed_grads.items() if n > 0]
        for k in cls.packed_grads:
            cls.packed_uses.pop(k, None)
        cls.packed_grads.clear()
        if left:
            raise RuntimeError(f"PoeReparamKL: {len(left)} head output(s) were read by more column-range fusion calls than "
                               f"took part in this backward pass; their gradient was not delivered "
                               f"(ops.GradReducer.share_packed_grads = False restores one gradient tensor per call)")
    merge_adjacent = True      # (module switch for the tests: False = one table entry per registered segment)

    # dw_jobs: weight gradients of Linear layers whose backward only launched the data gradient (Linear.backward, while
    # `early_step` is armed, on the fusion's stream): (dy, x, dw, db, M, N, K, x_act), tensors held until flush_dw queues them
    dw_jobs = []
    dw_open = False       # True from the arming of `early_step` until EarlyStepPoint.backward has queued the parked jobs
    dw_later_enabled = os.environ.get("MMVAE_LINEAR_DW_LATER", "1") == "1"

    # data_ptr of a preset gradient view -> stream of the launch that last accumulated into it IN PLACE this step
    last_writer = {}

    @classmethod
    def writes(cls, device, *grads):
        """The launch the caller queues next on the current stream accumulates in place (read-modify-write, no atomics)
        into these preset gradient views -- the small layers whose weight gradient needs no split partials.  Two calls of
        ONE module on different streams (POE._decoder_lanes: the text decoder at full length beside the same decoder under
        the mask) would race on them: the later launch (host order = autograd order) first waits for the stream of the
        earlier one.  No-op while a parameter is only ever written from one stream (every other step of this package)."""
        if device.type != "cuda":
            return
        cur = torch.cuda.current_stream(device)
        for g in grads:
            if g is None:
                continue
            k = g.data_ptr()
            last = cls.last_writer.get(k)
            if last is not None and last != cur:
                cur.wait_stream(last)
            cls.last_writer[k] = cur

    @classmethod
    def dw_later(cls, device):
        es = cls.early_step
        return (cls.dw_later_enabled and cls.dw_open and es is not None and torch.cuda.current_stream(device) == es[1]
                and len(cls.dw_jobs) < H.WGRAD_BATCH_MAX)

    @classmethod
    def flush_dw(cls):
        """the parked weight gradients in one launch on the current stream (every job direct into the flat gradient)"""
        jobs, cls.dw_jobs = cls.dw_jobs, []
        if not jobs:
            return
        arr = (H.WgradJob * len(jobs))()
        cls.writes(jobs[0][0].device, *[t for job in jobs for t in job[2:4]])
        for j, (dy, x, dw, db, M, N, K, x_act) in zip(arr, jobs):
            j.dy, j.x, j.dw, j.db, j.ws = H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), None
            j.M, j.N, j.K, j.ldx, j.x_act, j.accumulate = M, N, K, K, x_act, H.ACC_DEFER
        _call("mmvae_linear_bwd_weight_batch", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())

    # cw_jobs: weight gradients of Dec_CNN's two large ConvTranspose2d layers (32 -> 3 on the 32 x 32 map, 32 -> 32 on the
    # 16 x 16 one) whose backward only launched the data gradient (_convT_k4s2_bwd): (x, dy, dw, db, ws, (B, Cin, Cout, Hin),
    # x_act), tensors held until flush_cw has queued them as ONE launch.  Nothing on the chain image decoder -> fusion ->
    # encoders reads dW / db -- their first reader is the optimiser launch that folds the decoders' range -- so the launch
    # runs on the OTHER stream of the step, behind the text decoder's backward pass (cw_streams, set by
    # MoPOE.objective_backward for a captured one-GPU step: (the fusion's stream, the other decoder's)).
    cw_jobs = []
    cw_enabled = os.environ.get("MMVAE_CONV_DW_LATER", "1") == "1"
    # largest batch at which a layer is parked (same box, cfg2 step, parent -> parked, DESIGN.md 0 and
    # profiles/r07_conv_dw_later.txt): beside the chain's latency-bound kernels the launch costs what it occupies of the chip
    CW_MAX_BATCH = {(32, 3, 32): 128, (32, 32, 16): 64}
    cw_streams = None
    cw_done = None        # event behind the batch launch; EarlyStepPoint.backward (or the end-of-backward join) waits for it

    @classmethod
    def cw_later(cls, device, shape):
        st = cls.cw_streams
        return (cls.cw_enabled and st is not None and torch.cuda.current_stream(device) == st[0]
                and shape[0] <= cls.CW_MAX_BATCH.get(tuple(shape[1:]), 0) and len(cls.cw_jobs) < H.CONV_WGRAD_BATCH_MAX)

    @classmethod
    def cw_park(cls, job):
        """-> None, or (the last layer of this batch size is parked) the function that queues the batch launch; the caller
        calls it BEHIND its own data-gradient launch: captured in the other order, the graph holds the chain's next kernel
        back until the batch launch starts (profiles/r07_conv_dw_later.txt).  The launch waits for what the chain has
        queued up to HERE: the data gradient that produced this job's dy."""
        cls.cw_jobs.append(job)
        B = job[5][0]
        if len(cls.cw_jobs) < sum(B <= m for m in cls.CW_MAX_BATCH.values()):
            return None
        dev = job[0].device
        ev = torch.cuda.current_stream(dev).record_event()
        return lambda: cls._cw_launch(dev, ev)

    @classmethod
    def _cw_launch(cls, dev, ev):
        side = cls.cw_streams[1]
        side.wait_event(ev)
        for j in cls.cw_jobs:
            for t in j[:2]:      # x, dy: allocated on the chain's stream, read on the other one
                (t._base if t._base is not None else t).record_stream(side)
        with torch.cuda.stream(side):
            cls.flush_cw()
            cls.cw_done = side.record_event()
        cls.note_stream(dev, side)      # (the end-of-backward join covers a step without EarlyStepPoint)

    @classmethod
    def flush_cw(cls):
        """the parked conv weight gradients in one launch on the current stream (partials into their arena slices)"""
        jobs, cls.cw_jobs = cls.cw_jobs, []
        if not jobs:
            return
        arr = (H.ConvWgradJob * len(jobs))()
        for j, (x, dy, dw, db, ws, (B, Cin, Cout, Hin), x_act) in zip(arr, jobs):
            j.x, j.dy, j.ws = H.ptr(x), H.ptr(dy), H.ptr(ws)
            j.B, j.Cin, j.Cout, j.Hin, j.x_act, j.has_bias = B, Cin, Cout, Hin, x_act, int(db is not None)
        _call("mmvae_conv_wgrad_batch", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())

    # tw_jobs: {stream: [(dy2, x2, w, b, gw, gb)]} -- weight gradients of TALL-SKINNY Linear layers (the action towers'
    # attention projections: 12 800 rows, 32 .. 96 columns) whose backward only launched the data gradient.  Eight of them
    # share one launch of the tall-skinny weight-gradient kernel (_txt_wgrad: csrc/twgrad.hip) on the stream they were
    # parked from; what is left goes out at the end of the backward pass, in front of the join.  Alone, 12 800 x 96 x 32:
    # grouped data + weight launch 11.5 us; data gradient 4.8 + 22.1 / 8 per job (tools/probe/skinny_time.py).
    tw_jobs = {}
    tw_enabled = os.environ.get("MMVAE_SKINNY_DW", "1") == "1"
    TW_MIN_ROWS, TW_MAX_N, TW_MAX_K = 2048, 162, 128

    @classmethod
    def tw_ok(cls, M, N, K, in_act, has_b, dy, x):
        return (cls.tw_enabled and M >= cls.TW_MIN_ROWS and N <= cls.TW_MAX_N and K <= cls.TW_MAX_K and in_act == H.ACT_NONE
                and has_b and TXT_WGRAD and dy.is_contiguous() and x.is_contiguous()
                and H.lib().mmvae_txt_wgrad_supported(M, N, K))

    @classmethod
    def tw_park(cls, job):
        dev = job[0].device
        st = torch.cuda.current_stream(dev)
        lst = cls.tw_jobs.setdefault(st, [])
        lst.append(job)
        cls.note_stream(dev, st)
        cls.ensure_flush(dev)
        if len(lst) >= H.TXT_WGRAD_MAX:
            cls.tw_jobs[st] = []
            _txt_wgrad(lst)

    @classmethod
    def tw_flush_stream(cls, st):
        lst = cls.tw_jobs.pop(st, None)
        if lst:
            _txt_wgrad(lst)      # (on the current stream == st)

    @classmethod
    def tw_flush(cls):
        jobs, cls.tw_jobs = cls.tw_jobs, {}
        for st, lst in jobs.items():
            if lst:
                with torch.cuda.stream(st):
                    _txt_wgrad(lst)

    @classmethod
    def run_early_step(cls, device):
        es = cls.early_step
        if es is None or not cls.early_ready:
            return
        fn, stream, lo, hi = es
        _, st = cls._st(device)
        if torch.cuda.current_stream(device) != stream:      # (another tower's launch of the same kind)
            return
        cls.early_step = None
        if st["spill"] or not cls.defer_next:
            return
        inside = cls._merged([sg for sg in st["segs"] if lo <= sg[1] < hi])
        if len(inside) > H.MAX_SEGMENTS or any(sg[1] + 4 * sg[3] > hi for sg in inside):
            return
        st["segs"] = [sg for sg in st["segs"] if not (lo <= sg[1] < hi)]
        assert cls.cw_done is None      # (EarlyStepPoint.backward has ordered the parked conv weight gradients in front)
        # (no parked weight gradient is left here: EarlyStepPoint.backward, which sets `early_ready`, has queued them all
        # and closed `dw_open`)
        fn(cls._table(inside) if inside else None)

    @classmethod
    def keep(cls, device, *tensors):
        """hold tensors that a side-stream kernel still reads until the end-of-backward join"""
        cls._st(device)[1]["keep"].extend(t for t in tensors if t is not None)

    @classmethod
    def note_stream(cls, device, stream):
        cls._st(device)[1]["used"].add(stream)

    @classmethod
    def ensure_flush(cls, device):
        """queue the end-of-backward flush (side-stream join) even when no split partials were registered"""
        _, st = cls._st(device)
        if not st["armed"]:
            st["armed"] = True
            torch.autograd.Variable._execution_engine.queue_callback(lambda: cls.flush(device))

    @classmethod
    def flush(cls, device):
        cls.flush_dw()      # (no EarlyStepPoint ran behind them: here, behind the whole backward pass)
        cls.flush_cw()      # (a batch whose last layer never came)
        cls.tw_flush()      # (each list on the stream it was parked from, in front of the join below)
        _, st = cls._st(device)
        cur = torch.cuda.current_stream(device)
        if cls.pre_join is not None:
            cls.pre_join(device, [s_ for s_ in st["used"] if s_ != cur])
        for side in st["used"]:               # join every side stream that carried gradient work
            if side != cur:
                cur.wait_stream(side)
        st["used"] = set()
        st["keep"] = []
        segs, st["segs"], st["armed"] = cls._merged(st["segs"]), [], False
        cls._check_disjoint(segs)
        need, st["off"] = st["spilled"] + st["off"], 0
        tail, cls.tail = cls.tail, None
        defer, cls.defer_next = cls.defer_next, False
        if defer and 0 < len(segs) <= H.MAX_SEGMENTS and not st["spill"]:
            cls.deferred = {"table": cls._table(segs), "tail": tail, "device": device}
            if tail is not None:
                tail["done"] = True          # filled by the optimiser's launch
            return
        for i in range(0, len(segs), H.MAX_SEGMENTS):
            t = cls._table(segs[i:i + H.MAX_SEGMENTS])
            if tail is not None and i + H.MAX_SEGMENTS >= len(segs):
                # the logged loss values ride on the last fold launch as one extra workgroup
                rp, flat, out, n, B, k = tail["args"]
                _call("mmvae_reduce_segments_lincomb", ctypes.byref(t), ctypes.byref(rp), flat, H.ptr(out), n, B, k,
                      H.stream())
                tail["done"] = True
            else:
                _call("mmvae_reduce_segments", ctypes.byref(t), H.stream())
        if st["spill"]:        # the step did not fit one chunk: one arena of the full size from the next step on
            st["spill"], st["spilled"] = [], 0
            if not torch.cuda.is_current_stream_capturing():
                cls._arena[H.device_key(device)] = torch.empty(need + (1 << 20), dtype=torch.float32, device=device)


class Marks:
    """debug phase markers (MMVAE_MARKS=1): device wall-clock stamps in stream order, see tools/phase_timeline.py"""
    enabled = os.environ.get("MMVAE_MARKS", "0") == "1"
    names = []
    buf = None

    @classmethod
    def mark(cls, name):
        if not cls.enabled:
            return
        if cls.buf is None:
            cls.buf = torch.zeros(256, dtype=torch.int64, device="cuda")
        if name not in cls.names:
            cls.names.append(name)
        i = cls.names.index(name)
        _call("mmvae_debug_timestamp", cls.buf.data_ptr() + 8 * i, H.stream())


class Mark(Function):
    """identity that stamps `fwd:name` in forward and `bwd:name` in backward (on the stream each runs on)"""

    @staticmethod
    def forward(ctx, x, name):
        ctx.name = name
        Marks.mark("fwd:" + name)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        Marks.mark("bwd:" + ctx.name)
        return g, None


def mark_tensor(x, name):
    return Mark.apply(x, name) if Marks.enabled else x


class StreamPlan:
    """Overlap on separate HIP streams (captured into one hipGraph as parallel branches).

    At batch 128 every kernel of the step is far too small to fill 256 CUs, so the step time is the length of the
    dependency chain.  One independent chain is taken off the critical path: the text tower (encoder / decoder, forward
    and backward) runs beside the image tower.  Side streams are forked with events from the stream that produced their
    inputs and joined before the deferred reduction (GradReducer.flush) / at the fusion and loss points in the mixers."""

    # Measured on MI355X / ROCm 7.2, B=128: parallel graph branches DO overlap, but every
    # fork/join costs several microseconds, so only coarse forks pay:
    #   MMVAE_STREAMS=0         1.30 ms/step   single stream
    #   MMVAE_STREAMS=tower     0.99 ms/step   (default) text tower beside image tower: 2 forks + 2 joins per step
    # (weight gradients on side streams of their own -- the former values batch / conv / 1 -- were slower: 1.06 / 1.20 /
    # 1.30 ms/step, removed)
    _mode = os.environ.get("MMVAE_STREAMS", "tower")
    if _mode not in ("0", "tower"):
        raise ValueError(f"MMVAE_STREAMS={_mode!r}: accepted values are '0' (one stream) and 'tower' (default)")
    enabled = _mode == "tower"
    # (measured and removed in round 2, DESIGN.md 5b: a conv layer's backward as a data-gradient launch on the tower's
    # stream + a weight-gradient launch on a third stream -- 0.634 ms/step, the graph serialises; and the small-map
    # layers' fused backward as two launches on the same stream -- 0.450 / 0.457 / 0.489 ms for maps <= 4 / 8 / 16)
    _streams = {}

    @classmethod
    def get(cls, kind, device):
        key = (kind, H.device_key(device))
        s = cls._streams.get(key)
        if s is None:
            s = torch.cuda.Stream(device=device)
            cls._streams[key] = s
        return s

    pair = {}      # device key -> (capture stream, tower side stream) of the step being built (mixers set / clear it)

    @classmethod
    def other_stream(cls, device):
        """the step's stream that is NOT the current one (None outside a two-stream step)"""
        pr = cls.pair.get(H.device_key(device))
        if not pr:
            return None
        cur = torch.cuda.current_stream(device)
        if cur == pr[0]:
            return pr[1]
        if cur == pr[1]:
            return pr[0]
        return None


def _defer(*grads):
    """deferred reduction applies when the op accumulates into preset (flat) gradient views"""
    return GradReducer.enabled and all(g is not None for g in grads)


class DropSpec:
    """One dropout application: (state tensor, slot, site, p) -> the C struct, plus an optional recorder used by the
    tests to extract the very masks a forward pass used."""
    recorder = None     # list collecting (name, state, slot, site, p, n) when set

    def __init__(self, state, slot, site, p, name=""):
        self.state, self.slot, self.site, self.p, self.name = state, int(slot), int(site), float(p), name

    def c(self):
        return ctypes.byref(H.Dropout(self.state.data_ptr(), self.slot, self.site, self.p))

    def note(self, n):
        if DropSpec.recorder is not None:
            DropSpec.recorder.append((self.name, self.state, self.slot, self.site, self.p, int(n)))


def _dp(drop, n=0):
    if drop is None:
        return None
    drop.note(n)
    return drop.c()


def dropout_advance(state, slot):
    _call("mmvae_dropout_advance", H.ptr(state), int(slot), H.stream())


def dropout_advance_many(states):
    """dropout_advance(st, 0) for every state tensor in `states` (distinct towers) in one launch"""
    arr = (ctypes.c_void_p * len(states))(*[H.ptr(t) for t in states])
    _call("mmvae_dropout_advance_many", ctypes.cast(arr, ctypes.c_void_p), len(states), H.stream())


def dropout_mask(drop, n):
    out = torch.empty(n, device=drop.state.device)
    _call("mmvae_dropout_mask", drop.c(), H.ptr(out), n, H.stream())
    return out


def _new_like_param(p, g):
    """(destination tensor, accumulate flag, value to hand back to autograd)"""
    if g is not None:
        return g, 1, None
    t = torch.empty_like(p)
    return t, 0, t


def _grad_dst(w, gw, gb, has_b, n_bias):
    """destinations of a layer's weight and bias gradient: (dw, db, accumulate flag of dw, the two values to hand back to
    autograd).  db is the preset view `gb`, a fresh (n_bias,) tensor, or None for a layer without bias."""
    dw, acc_w, ret_w = _new_like_param(w, gw)
    db = ret_b = None
    if has_b:
        db = gb
        if gb is None:
            db = ret_b = torch.empty(n_bias, device=w.device)
    return dw, db, acc_w, ret_w, ret_b


# ----------------------------------------------------------------------------------------------
# convolutions
# ----------------------------------------------------------------------------------------------
class Conv2dK4S2(Function):
    """y = conv2d(act(x), w, b, stride 2, pad 1)   [nn.Conv2d, models/encoders.py:186-191,214-217]"""

    @staticmethod
    def forward(ctx, x, w, b, in_act, gw, gb):
        x = H.f32c(x)
        B, Cin, Hin, _ = x.shape
        Cout = w.shape[0]
        y = torch.empty(B, Cout, Hin // 2, Hin // 2, device=x.device, dtype=torch.float32)
        _call("mmvae_conv2d_k4s2_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), B, Cin, Cout, Hin, in_act,
              H.EP_NONE, H.stream())
        ctx.save_for_backward(x, w)
        ctx.cfg = (in_act, gw, gb, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        in_act, gw, gb, has_b = ctx.cfg
        dy = H.f32c(dy)
        B, Cin, Hin, _ = x.shape
        Cout, Hout = w.shape[0], Hin // 2
        dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, has_b, Cout)
        nws = H.lib().mmvae_conv_wgrad_ws_floats(B, Cout, Cin, Hout)
        defer = _defer(gw, gb if has_b else gw)
        ws = GradReducer.alloc(nws, x.device) if defer else H.workspace(nws, x.device)
        acc = H.ACC_DEFER if defer else acc_w
        dx = None
        if ctx.needs_input_grad[0]:       # input- and weight-gradient workgroups in ONE launch
            dx = torch.empty_like(x)
            _call("mmvae_conv2d_k4s2_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
                  B, Cin, Cout, Hout, in_act, acc, H.stream())
        else:
            _call("mmvae_conv2d_k4s2_wgrad", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), H.ptr(ws), B, Cin, Cout, Hout,
                  in_act, acc, H.stream())
        if defer:
            _conv_segments(ws, dw, db, B, Cout, Cin, Hout, Cout)
        return dx, ret_w, ret_b, None, None, None


class ConvT2dK4S2(Function):
    """y = ep(conv_transpose2d(act(x), w, b, stride 2, pad 1))   [nn.ConvTranspose2d, models/decoders.py:62-69,91-97]
    out_ep: EP_NONE or EP_SIGMOID_CLAMP (decoders.py:96-97)."""

    @staticmethod
    def forward(ctx, x, w, b, in_act, out_ep, gw, gb, ep_bwd=True):
        """ep_bwd False: the incoming gradient is already the gradient of the PRE-epilogue value (see SigmoidClampOut)"""
        x = H.f32c(x)
        B, Cin, Hin, _ = x.shape
        Cout = w.shape[1]
        y = torch.empty(B, Cout, 2 * Hin, 2 * Hin, device=x.device, dtype=torch.float32)
        _call("mmvae_convT2d_k4s2_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), B, Cin, Cout, Hin, in_act,
              out_ep, H.stream())
        if not ep_bwd:
            out_ep = H.EP_NONE
        ctx.save_for_backward(x, w, y if out_ep in (H.EP_SIGMOID_CLAMP, H.EP_SIGMOID) else None)
        ctx.cfg = (in_act, out_ep, gw, gb, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        in_act, out_ep, gw, gb, has_b = ctx.cfg
        dy = H.f32c(dy)
        B, Cin, Hin, _ = x.shape
        Cout = w.shape[1]
        if out_ep == H.EP_SIGMOID_CLAMP:
            dl = torch.empty_like(dy)
            _call("mmvae_sigmoid_clamp_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
            dy = dl
        elif out_ep == H.EP_SIGMOID:
            dl = torch.empty_like(dy)
            _call("mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
            dy = dl
        dx, ret_w, ret_b = _convT_k4s2_bwd(x, w, dy, in_act, gw, gb, has_b, ctx.needs_input_grad[0])
        return dx, ret_w, ret_b, None, None, None, None, None


def _convT_k4s2_bwd(x, w, dy, in_act, gw, gb, has_b, need_dx):
    """dx, dw, db of y = convT2d(act(x), w, b) for dy = d loss / d y (ConvT2dK4S2.backward, ConvT3Bce.backward)"""
    B, Cin, Hin, _ = x.shape
    Cout = w.shape[1]
    dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, has_b, Cout)
    nws = H.lib().mmvae_conv_wgrad_ws_floats(B, Cin, Cout, Hin)
    defer = _defer(gw, gb if has_b else gw)
    ws = GradReducer.alloc(nws, x.device) if defer else H.workspace(nws, x.device)
    acc = H.ACC_DEFER if defer else acc_w
    dx = None
    if need_dx and defer and GradReducer.cw_later(x.device, (B, Cin, Cout, Hin)):
        # the captured one-GPU MoPoE step, one of the image decoder's two large layers: only the DATA gradient (the same
        # kernel and tile order as the fused launch's data-gradient part) sits on the chain decoder -> fusion -> encoders;
        # the parked weight gradients follow in ONE launch on the step's other stream (GradReducer.cw_park), same partials in `ws`
        dx = torch.empty_like(x)
        go = GradReducer.cw_park((x, dy, dw, db, ws, (B, Cin, Cout, Hin), in_act))
        ep = _DACT[in_act]
        _call("mmvae_convT2d_k4s2_dgrad", H.ptr(dy), H.ptr(w), H.ptr(x) if ep else None, H.ptr(dx), B, Cin, Cout, Hin, ep,
              H.stream())
        if go is not None:
            go()
    elif need_dx:       # input- and weight-gradient workgroups in ONE launch
        dx = torch.empty_like(x)
        _call("mmvae_convT2d_k4s2_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
              B, Cin, Cout, Hin, in_act, acc, H.stream())
    else:
        _call("mmvae_convT2d_k4s2_wgrad", H.ptr(x), H.ptr(dy), H.ptr(dw), H.ptr(db), H.ptr(ws), B, Cin, Cout, Hin,
              in_act, acc, H.stream())
    if defer:
        _conv_segments(ws, dw, db, B, Cin, Cout, Hin, Cout)
    return dx, ret_w, ret_b


_T3_SCRATCH = {}      # (device, stream, B) -> (partial sums (B, strips), tickets (B)) of ConvT3Bce


class ConvT3Bce(Function):
    """Dec_CNN's last layer AND its reconstruction term in one launch (csrc/conv_t3.inc):
    row[b] = sum bce(clamp(sigmoid(convT2d(act(x), w, b)))[b], target[b])   [models/decoders.py:69,95-97 +
    ReconLoss.bce, models/objectives.py:392-406].  Only under ops.ConstSeed (the term's ELBO weight is known): the same
    pass writes d loss / d logits, x_hat itself is never stored.  Backward = the layer's ordinary backward on that."""

    calls = 0      # (tests: how often the fused form ran)

    @staticmethod
    def forward(ctx, x, w, b, in_act, gw, gb, target, cs):
        ConvT3Bce.calls += 1
        x, target = H.f32c(x), H.f32c(target)
        B = x.shape[0]
        dev = x.device
        row = torch.empty(B, device=dev)
        dl = torch.empty(B, 3, 64, 64, device=dev)
        S = H.lib().mmvae_convT3_bce_strips(B)
        part = tick = None
        if S > 1:
            key = (dev.index, H.stream(), B)
            ent = _T3_SCRATCH.get(key)
            if ent is None:      # (first call = a warm-up pass: no allocation / memset node under graph capture)
                # a first call INSIDE a capture would put the buffers into the graph's private pool and the
                # memset into the graph, while this cache hands them to eager calls as well
                assert not torch.cuda.is_current_stream_capturing(), \
                    "ConvT3Bce: first call at this batch size inside a graph capture (run one eager warm-up step first)"
                ent = _T3_SCRATCH[key] = (torch.zeros(B * S, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
            part, tick = ent
        _call("mmvae_convT3_bce_seeded", H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(target), H.ptr(row), H.ptr(dl), H.ptr(part),
              H.ptr(tick), B, in_act, cs.value, H.stream())
        ctx.save_for_backward(x, w, dl)
        ctx.cfg = (in_act, gw, gb, b is not None, cs.seed.data_ptr(), cs.value)
        return row

    @staticmethod
    def backward(ctx, g):
        x, w, dl = ctx.saved_tensors
        in_act, gw, gb, has_b, seed_ptr, seed_value = ctx.cfg
        if g.data_ptr() != seed_ptr:      # not the announced upstream gradient: rescale the stored logit gradient per row
            dl = dl * (H.f32c(g) / seed_value).view(-1, 1, 1, 1)
        dx, ret_w, ret_b = _convT_k4s2_bwd(x, w, dl, in_act, gw, gb, has_b, ctx.needs_input_grad[0])
        return dx, ret_w, ret_b, None, None, None, None, None


CONVT3_BCE = True      # module switch (tests / A-B runs): False = last layer and bce loss as two launches


def convT3_bce_supported(x, w, target):
    # from 256 images on (<= 2 strips per image): same box, cfg2 step, fused vs two launches -- batch 128: 0.3866 vs 0.3852 ms
    # (four strips per image, the ticketed row sum and the loss arithmetic on 512 short workgroups buy nothing), batch 1000:
    # 1.5025 vs 1.5372 (profiles/r05_convT3_ab.txt)
    # (an ELBO weight of 0 -- llik_scaling 0 -- leaves no way to rescale the stored logit gradient: two launches then)
    return (CONVT3_BCE and x.shape[0] >= 256 and ConstSeed.current is not None and ConstSeed.current.value != 0 and
            x.is_cuda and x.dim() == 4 and tuple(x.shape[1:]) == (32, 32, 32) and
            tuple(w.shape) == (32, 3, 4, 4) and target.numel() == x.shape[0] * 3 * 64 * 64 and x.requires_grad)


def convT3_bce(x, w, b, in_act, gw, gb, target):
    return ConvT3Bce.apply(x, w, b, in_act, gw, gb, target, ConstSeed.current)


class SigmoidClampOut(Function):
    """Identity on the forward values of a layer whose kernel already applied clamp(sigmoid(.)); in backward it turns
    the gradient of that output into the gradient of the logits.  Splitting the epilogue's backward off the layer
    lets a loss that knows the logits' gradient in closed form (BceSigmoidRowsum) feed the layer directly."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = H.f32c(dy)
        dl = torch.empty_like(dy)
        _call("mmvae_sigmoid_clamp_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
        return dl


class ConstSeed:
    """`with ConstSeed(seed, value):` -- the loss rows created inside are known to receive the persistent tensor `seed`
    (every element == `value`: the ELBO is linear in them) as their upstream gradient.  Their forward kernels then
    write the input gradient in the same pass and backward hands it out without a launch when it is indeed called
    with `seed` (any other upstream gradient takes the ordinary backward kernel)."""
    current = None

    def __init__(self, seed, value):
        self.seed, self.value = seed, float(value)

    def __enter__(self):
        self.prev, ConstSeed.current = ConstSeed.current, self
        return self

    def __exit__(self, *exc):
        ConstSeed.current = self.prev


class BceSigmoidRowsum(Function):
    """BceRowsum on x_hat = clamp(sigmoid(logits)) given as the layer's raw output (whose gradient is taken with
    respect to the LOGITS): backward is the closed form g (x_hat - t) [clamp inactive] in one kernel."""

    @staticmethod
    def forward(ctx, y_raw, target):
        """target: (B, ...) or, for a K-sample output, (B / K, ...) -- output row r is paired with target row
        r % (B / K) (the repeat of BaseObjective.reshape_for_loss, objectives.py:118-120, is never materialised)"""
        y_raw, target = H.f32c(y_raw), H.f32c(target)
        B = y_raw.shape[0]
        F_ = y_raw.numel() // B
        trows = target.numel() // F_
        assert trows * F_ == target.numel() and B % trows == 0
        row = torch.empty(B, device=y_raw.device)
        cs = ConstSeed.current
        ctx.seeded = None
        if cs is not None and y_raw.requires_grad and trows == B:
            dl = torch.empty_like(y_raw)
            _call("mmvae_bce_rowsum_seeded", H.ptr(y_raw), H.ptr(target), H.ptr(row), cs.value, H.ptr(dl), B, F_,
                  H.stream())
            ctx.seeded = (cs.seed.data_ptr(), dl)
        else:
            _call("mmvae_bce_rowsum_fwd", H.ptr(y_raw), H.ptr(target), H.ptr(row), B, F_, trows, H.stream())
        ctx.save_for_backward(y_raw, target)
        ctx.trows = trows
        return row

    @staticmethod
    def backward(ctx, g):
        if ctx.seeded is not None and g.data_ptr() == ctx.seeded[0]:
            return ctx.seeded[1], None
        y, target = ctx.saved_tensors
        B = y.shape[0]
        dl = torch.empty_like(y)
        _call("mmvae_bce_sigmoid_clamp_bwd", H.ptr(y), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(dl), B, y.numel() // B,
              ctx.trows, H.stream())
        return dl, None


class ConvGeneric(Function):
    """Conv2d (transposed = False) or ConvTranspose2d (True) with any channel counts, K <= 4, stride, padding, on the
    generic kernels of csrc/conv_generic.hip (Enc_SVHN / Dec_SVHN layers outside the k4-s2-p1 3/32-channel shapes)."""

    @staticmethod
    def forward(ctx, x, w, b, transposed, stride, pad, in_act, out_ep, gw, gb):
        x = H.f32c(x)
        B, Cin, Hin, Win = x.shape
        K = w.shape[-1]
        if transposed:
            Cout = w.shape[1]
            Ho, Wo = (Hin - 1) * stride - 2 * pad + K, (Win - 1) * stride - 2 * pad + K
        else:
            Cout = w.shape[0]
            Ho, Wo = (Hin + 2 * pad - K) // stride + 1, (Win + 2 * pad - K) // stride + 1
        y = torch.empty(B, Cout, Ho, Wo, device=x.device)
        _call("mmvae_convT2d_generic_fwd" if transposed else "mmvae_conv2d_generic_fwd", H.ptr(x), H.ptr(w), H.ptr(b),
              None, H.ptr(y), B, Cin, Cout, Hin, Win, K, stride, pad, in_act, out_ep, H.stream())
        ctx.save_for_backward(x, w, y if out_ep in (H.EP_SIGMOID_CLAMP, H.EP_SIGMOID) else None)
        ctx.cfg = (transposed, stride, pad, in_act, out_ep, gw, gb, b is not None, Cout)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        transposed, stride, pad, in_act, out_ep, gw, gb, has_b, Cout = ctx.cfg
        dy = H.f32c(dy)
        B, Cin, Hin, Win = x.shape
        K = w.shape[-1]
        if out_ep in (H.EP_SIGMOID_CLAMP, H.EP_SIGMOID):
            dl = torch.empty_like(dy)
            _call("mmvae_sigmoid_clamp_bwd" if out_ep == H.EP_SIGMOID_CLAMP else "mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y),
                  H.ptr(dl), dy.numel(), H.stream())
            dy = dl
        dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, has_b, Cout)
        pre = "mmvae_convT2d_generic" if transposed else "mmvae_conv2d_generic"
        _call(pre + "_wgrad", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), B, Cin, Cout, Hin, Win, K, stride, pad, in_act,
              acc_w, H.stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ep = _DACT[in_act]
            _call(pre + "_dgrad", H.ptr(dy), H.ptr(w), H.ptr(x) if ep else None, H.ptr(dx), B, Cin, Cout, Hin, Win, K,
                  stride, pad, ep, H.stream())
        return dx, ret_w, ret_b, None, None, None, None, None, None, None


def _pow2(v, lo, hi):
    return lo <= v <= hi and (v & (v - 1)) == 0


def _mfma_conv_shape(c_gather_red, c_out32, h_big):
    """shapes the MFMA 4x4 / stride-2 / pad-1 kernels are instantiated for, in the gather orientation (big map h_big
    with `c_gather_red` channels <-> small map h_big / 2 with `c_out32` channels, a multiple of 32): the CdSprites+
    towers' 3 / 32-channel layers and the SVHN towers' 64-channel layers"""
    if c_out32 % 32 or c_out32 > 128:
        return False
    if c_gather_red == 3:
        return c_out32 == 32 and _pow2(h_big, 8, 64)
    if c_gather_red == 32:
        return _pow2(h_big, 8, 32)
    if c_gather_red == 64:
        return _pow2(h_big, 8, 16)
    return False


def conv2d(x, w, b, stride=2, pad=1, in_act=H.ACT_NONE, gw=None, gb=None):
    """nn.Conv2d on act(x): the MFMA kernels for the k4-s2-p1 layers (3 / 32 / 64 -> 32 / 64 channels), a plain GEMM
    when the kernel covers the whole map (SVHN conv4: k4 s2 p0 on 4x4 -> 1x1), the generic kernel otherwise"""
    Cout, Cin, K, _ = w.shape
    Hin = x.shape[-1]
    if K == 4 and stride == 2 and pad == 1 and x.shape[-2] == Hin and _mfma_conv_shape(Cin, Cout, Hin):
        return Conv2dK4S2.apply(x, w, b, in_act, gw, gb)
    if pad == 0 and x.shape[-2] == K and Hin == K:      # one output position: y[b, o] = <act(x[b]), w[o]> + bias[o]
        B = x.shape[0]
        y = Linear.apply(x.reshape(B, Cin * K * K), w.view(Cout, Cin * K * K), b, in_act,
                         gw.view(Cout, Cin * K * K) if gw is not None else None, gb)
        return y.view(B, Cout, 1, 1)
    return ConvGeneric.apply(x, w, b, False, stride, pad, in_act, H.EP_NONE, gw, gb)


def convT2d(x, w, b, stride=2, pad=1, in_act=H.ACT_NONE, out_ep=H.EP_NONE, gw=None, gb=None, ep_bwd=True):
    """nn.ConvTranspose2d on act(x), optional sigmoid epilogue: MFMA kernels for the k4-s2-p1 layers, a plain GEMM for a
    1x1 input (SVHN decoder conv1: k4 s1 p0, 1x1 -> 4x4), the generic kernel otherwise"""
    Cin, Cout, K, _ = w.shape
    Hin = x.shape[-1]
    if K == 4 and stride == 2 and pad == 1 and x.shape[-2] == Hin:
        if Cout == 3 and Cin == 32 and Hin in (16, 32):
            return ConvT2dK4S2.apply(x, w, b, in_act, out_ep, gw, gb, ep_bwd)
        if out_ep == H.EP_NONE and Cin in (32, 64) and _mfma_conv_shape(Cout, Cin, 2 * Hin) and Hin >= 4:
            return ConvT2dK4S2.apply(x, w, b, in_act, out_ep, gw, gb)
    if Hin == 1 and x.shape[-2] == 1 and pad == 0 and out_ep == H.EP_NONE:
        return LinearKN.apply(x.reshape(x.shape[0], Cin), w, b, in_act, gw, gb).view(x.shape[0], Cout, K, K)
    y = ConvGeneric.apply(x, w, b, True, stride, pad, in_act, out_ep, gw, gb)
    # (the generic kernel applies its epilogue's backward itself: undo that when the caller feeds logit gradients)
    assert ep_bwd or out_ep == H.EP_NONE, "ep_bwd=False needs an MFMA-kernel shape"
    return y


_conv_layouts = {}


def _conv_segments(ws, dw, db, B, c_small, c_large, h_small, n_bias):
    # (the layout of the partial rows is a pure function of the shape: a host-side query, asked once per shape -- it used
    # to be repeated on every backward pass and was counted among the step's C-ABI calls, 8 of cfg2's 54)
    key = (B, c_small, c_large, h_small)
    lay = _conv_layouts.get(key)
    if lay is None:
        rows, rowlen, bias_col = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        H.check(H.lib().mmvae_conv_wgrad_layout(B, c_small, c_large, h_small, ctypes.byref(rows), ctypes.byref(rowlen),
                                                ctypes.byref(bias_col)), "mmvae_conv_wgrad_layout")
        lay = _conv_layouts[key] = (rows.value, rowlen.value, bias_col.value)
    rows, rowlen, bias_col = lay
    GradReducer.add(ws.data_ptr(), dw, rows, dw.numel(), rowlen)
    if db is not None:
        GradReducer.add(ws.data_ptr() + 4 * bias_col, db, rows, n_bias, rowlen)


def conv2d_k4s2(x, w, b, in_act=H.ACT_NONE, gw=None, gb=None):
    return Conv2dK4S2.apply(x, w, b, in_act, gw, gb)


def convT2d_k4s2(x, w, b, in_act=H.ACT_NONE, out_ep=H.EP_NONE, gw=None, gb=None, ep_bwd=True):
    return ConvT2dK4S2.apply(x, w, b, in_act, out_ep, gw, gb, ep_bwd)


def sigmoid_clamp_out(y_raw):
    return SigmoidClampOut.apply(y_raw)


def bce_sigmoid_rowsum(y_raw, target):
    return BceSigmoidRowsum.apply(y_raw, target)


# ----------------------------------------------------------------------------------------------
# dense
# ----------------------------------------------------------------------------------------------
# y = norm(sub(x) + x): hand the residual branch's gradient to the sub-layer's first backward kernel (below)
RESIDUAL_HANDOFF = True


class ResidualGrad:
    """Side channel for the gradient of a residual connection y = LayerNorm(sub(x) + x).  Autograd would return the
    LayerNorm's residual gradient and the sub-layer's input gradient separately and add them in an elementwise launch of
    its own (24 per step of the trimodal workload).  Instead the LayerNorm's backward -- which runs first: the sub-layer
    feeds it -- leaves its residual gradient HERE and returns nothing for that input, and the backward of the sub-layer's
    FIRST op on x (ops.Linear: the attention in-projection; ops.Ffn32) adds it in its kernel's epilogue and returns the
    sum: the same gradient for x.  One object per residual connection, passed to both ops."""
    __slots__ = ("grad",)

    def __init__(self):
        self.grad = None

    def take(self):
        g, self.grad = self.grad, None
        return g


def residual_sink(x):
    """a ResidualGrad for a residual connection around x, or None when nothing is differentiated / the switch is off"""
    return ResidualGrad() if (RESIDUAL_HANDOFF and torch.is_grad_enabled() and x.requires_grad and x.is_cuda) else None


class Linear(Function):
    """y = act(x) W^T + b over the last dim   [nn.Linear / MHA projections / FFN]"""

    @staticmethod
    def forward(ctx, x, w, b, in_act, gw, gb, out_ep=H.EP_NONE, res_sink=None, lazy=False):
        """out_ep: EP_NONE, or EP_SIGMOID -- y = sigmoid(.) in the GEMM's epilogue; the incoming gradient is then
        taken as the gradient of the LOGITS (wrap the output in ops.sigmoid_out, see SigmoidOut).  res_sink: ResidualGrad.
        lazy: the output is a PLACEHOLDER (nothing is launched) -- its only consumer is a LayerNorm whose forward computes
        the product itself (ops.layernorm_residual(..., proj=...): mmvae_proj32_ln_fwd); backward is unchanged"""
        ctx.res_sink = res_sink
        x = H.f32c(x)
        K = x.shape[-1]
        M = x.numel() // K
        N = w.shape[0]
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        if not lazy:
            _call("mmvae_linear_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), M, N, K, K, in_act, out_ep, H.stream())
        ctx.save_for_backward(x, w)
        ctx.cfg = (in_act, gw, gb, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        in_act, gw, gb, has_b = ctx.cfg
        dy = H.f32c(dy)
        K = x.shape[-1]
        M = x.numel() // K
        N = w.shape[0]
        dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, has_b, N)
        need_dx = ctx.needs_input_grad[0]
        if dy.data_ptr() % 16:
            dy = dy.clone()
        lib = H.lib()
        nws = lib.mmvae_linear_bwd_ws_floats(M, N, K) if need_dx else lib.mmvae_linear_bwd_weight_ws_floats(M, N, K)
        dx = torch.empty_like(x) if need_dx else None
        ep = _DACT[in_act]
        aux = H.ptr(x) if ep else None
        radd = ctx.res_sink.take() if ctx.res_sink is not None else None      # the residual branch's gradient of x
        kadd = None
        if radd is not None and need_dx and not ep and radd.is_contiguous() and radd.numel() == x.numel():
            # ... added in the data gradient's epilogue; `kadd` keeps the tensor alive until the launch below is queued
            # (dropped before the launch, its block could be handed out again by any allocation in between)
            ep, aux, kadd, radd = H.EP_ADD_AUX, H.ptr(radd), radd, None
        defer = _defer(gw, gb if has_b else gw)
        nz = lib.mmvae_linear_bwd_splits(M, N, K) if need_dx else lib.mmvae_linear_bwd_weight_splits(M, N, K)
        if need_dx and defer and radd is None and GradReducer.tw_ok(M, N, K, in_act, has_b, dy, x):
            # tall-skinny layer: the data gradient now, the weight gradient with up to seven others in one launch of the
            # tall-skinny kernel (GradReducer.tw_park)
            _call("mmvae_linear_bwd_data", H.ptr(dy), H.ptr(w), aux, H.ptr(dx), M, N, K, ep, 0, H.stream())
            GradReducer.tw_park((dy.view(M, N), x.view(M, K), w, True, gw, gb))
            del kadd
            return dx, ret_w, ret_b, None, None, None, None, None, None
        if need_dx and defer and nz == 1 and radd is None and GradReducer.dw_later(x.device) and \
                lib.mmvae_linear_bwd_weight_splits(M, N, K) == 1:
            # the captured one-GPU MoPoE step, a Linear of the decoder that shares the fusion's stream: only the DATA
            # gradient sits on the critical chain decoder -> fusion -> encoders; the weight gradients of all such layers
            # follow in ONE launch behind the fusion's backward (GradReducer.flush_dw)
            _call("mmvae_linear_bwd_data", H.ptr(dy), H.ptr(w), aux, H.ptr(dx), M, N, K, ep, 0, H.stream())
            GradReducer.dw_jobs.append((dy, x, dw, db, M, N, K, in_act))
            del kadd
            return dx, ret_w, ret_b, None, None, None, None, None, None
        if defer:
            ws = GradReducer.alloc(nws, x.device) if nz > 1 else None
            acc = H.ACC_DEFER
        else:
            ws, acc = H.workspace(nws, x.device), acc_w
        direct = (gw, gb) if (gw is not None and not (defer and nz > 1)) else ()      # accumulated in place by the launch
        if need_dx:   # data and weight gradients in ONE grouped launch
            GradReducer.writes(x.device, *direct)
            _call("mmvae_linear_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), aux, H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
                  M, N, K, K, in_act, ep, acc, H.stream())
        else:
            GradReducer.writes(x.device, *direct)
            _call("mmvae_linear_bwd_weight", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), H.ptr(ws), M, N, K, K, in_act, acc,
                  H.stream())
        if defer and nz > 1:
            GradReducer.add(ws.data_ptr(), dw, nz, N * K, N * K)
            if db is not None:
                GradReducer.add(ws.data_ptr() + 4 * nz * N * K, db, nz, N, N)
        del kadd
        if radd is not None and dx is not None:
            dx = dx + radd.view_as(dx)
        return dx, ret_w, ret_b, None, None, None, None, None, None


PROJ32_LN = os.environ.get("MMVAE_PROJ32_LN", "1") == "1"      # out_proj + dropout + residual + LayerNorm in one launch (d = 32)


def linear(x, w, b, in_act=H.ACT_NONE, gw=None, gb=None, out_ep=H.EP_NONE, res_sink=None, lazy=False):
    y = Linear.apply(x, w, b, in_act, gw, gb, out_ep, res_sink, lazy)
    if lazy:
        y._proj = (x, w, b)      # what the consuming LayerNorm needs to compute the product itself
    return y


class SigmoidOut(Function):
    """Identity on the forward values of a layer whose kernel already applied sigmoid(.) in its epilogue (and whose
    backward takes the LOGITS' gradient); in backward it turns the gradient of that output into the gradient of the
    logits.  A loss that knows the logits' gradient in closed form (LprobRowsum, logit_grad) feeds the layer directly
    through the raw tensor (decoders set `out._lprob_src`)."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = H.f32c(dy)
        dl = torch.empty_like(dy)
        _call("mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
        return dl


def sigmoid_out(y_raw):
    return SigmoidOut.apply(y_raw)


class LinearKN(Function):
    """y[m, (c, g)] = sum_k act(x)[m, k] w[k, c, g] + b[c]  with the weight stored (K, C, kh, kw): nn.ConvTranspose2d
    (kernel = output size, stride 1, pad 0) on a 1x1 input -- the first layer of Dec_SVHN (models/decoders.py:116) --
    as plain strided GEMMs (forward, data gradient, weight gradient) + a grouped bias."""

    @staticmethod
    def forward(ctx, x, w, b, in_act, gw, gb):
        x = H.f32c(x)
        M, K = x.shape
        C = w.shape[1]
        G = w.shape[2] * w.shape[3]
        N = C * G
        y = torch.empty(M, N, device=x.device)
        _call("mmvae_gemm_f32", H.ptr(x), H.ptr(w), None, None, H.ptr(y), None, None, M, N, K, K, 1, N, 1, N, in_act,
              H.ACT_NONE, H.EP_NONE, 0, 1, H.stream())
        if b is not None:
            _call("mmvae_bias_group_add", H.ptr(y), H.ptr(b), M, C, G, H.stream())
        ctx.save_for_backward(x, w)
        ctx.cfg = (in_act, gw, gb, b is not None, C, G)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        in_act, gw, gb, has_b, C, G = ctx.cfg
        dy = H.f32c(dy)
        M, K = x.shape
        N = C * G
        lib = H.lib()
        dx = None
        if ctx.needs_input_grad[0]:       # dx[m, k] = ep( sum_n dy[m, n] w[k, n] )
            dx = torch.empty_like(x)
            ep = _DACT[in_act]
            _call("mmvae_gemm_f32", H.ptr(dy), H.ptr(w), None, H.ptr(x) if ep else None, H.ptr(dx), None, None, M, K, N,
                  N, 1, 1, N, K, H.ACT_NONE, H.ACT_NONE, ep, 0, 1, H.stream())
        # dw[k, n] (+)= sum_m act(x)[m, k] dy[m, n]: rows K, columns N, reduction over the M samples (split)
        dw, acc_w, ret_w = _new_like_param(w, gw)
        tiles = ((K + 31) // 32) * ((N + 31) // 32)
        want = max(1, min(64, 512 // max(tiles, 1), (M + 127) // 128))
        nz = lib.mmvae_gemm_splits(K, N, M, want)
        if nz <= 1:
            want, nz = 1, 1
        defer = _defer(gw) and nz > 1
        ws = None
        if nz > 1:
            nws = lib.mmvae_gemm_ws_floats(K, N, nz)
            ws = GradReducer.alloc(nws, x.device) if defer else H.workspace(nws, x.device)
        if gw is not None and not defer:
            GradReducer.writes(x.device, gw)
        _call("mmvae_gemm_f32", H.ptr(x), H.ptr(dy), None, None, H.ptr(dw), None, H.ptr(ws), K, N, M, 1, K, N, 1, N,
              in_act, H.ACT_NONE, H.EP_NONE, H.ACC_DEFER if defer else acc_w, want, H.stream())
        if defer:
            GradReducer.add(ws.data_ptr(), dw, nz, K * N, K * N)
        ret_b = None
        if has_b:
            nbw = lib.mmvae_bias_group_ws_floats(M, C)
            if _defer(gb):
                bws = GradReducer.alloc(nbw, x.device)
                _call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(gb), H.ptr(bws), M, C, G, H.ACC_DEFER, H.stream())
                GradReducer.add(bws.data_ptr(), gb, lib.mmvae_bias_group_parts(M), C, C)
            elif gb is not None:
                bws = torch.empty(nbw, device=x.device)
                GradReducer.writes(x.device, gb)
                _call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(gb), H.ptr(bws), M, C, G, 1, H.stream())
            else:
                ret_b = torch.empty(C, device=x.device)
                bws = torch.empty(nbw, device=x.device)
                _call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(ret_b), H.ptr(bws), M, C, G, 0, H.stream())
        return dx, ret_w, ret_b, None, None, None


# ----------------------------------------------------------------------------------------------
# ResNet-50 tower: global average pooling (csrc/rconv.hip); the rest of the tower is rconv.py / csrc/rconv.hip
# ----------------------------------------------------------------------------------------------
class AvgPoolGlobal(Function):
    """nn.AdaptiveAvgPool2d(1) on relu(x): (B*HW, C) -> (B, C)"""

    @staticmethod
    def forward(ctx, x, B, HW, in_act):
        x = H.f32c(x)
        C = x.shape[-1]
        y = torch.empty(B, C, device=x.device)
        _call("mmvae_avgpool_fwd", H.ptr(x), H.ptr(y), B, HW, C, in_act, H.stream())
        ctx.save_for_backward(x)
        ctx.cfg = (B, HW, C, in_act)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, HW, C, in_act = ctx.cfg
        dx = torch.empty_like(x)
        _call("mmvae_avgpool_bwd", H.ptr(H.f32c(dy)), H.ptr(x), H.ptr(dx), B, HW, C, in_act, H.stream())
        return dx, None, None, None


class HeadSoftmax(Function):
    """h (B,2D) = [mu | u]  ->  [mu | softmax(u)+1e-6]   (VaeComponent.process_output, models/encoders.py:49-54)"""

    @staticmethod
    def forward(ctx, h):
        assert h.is_contiguous() and h.dtype == torch.float32
        B, D2 = h.shape
        _call("mmvae_head_softmax_fwd", H.ptr(h), B, D2 // 2, H.stream())   # in place on the fresh linear output
        ctx.mark_dirty(h)
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, dh):
        (out,) = ctx.saved_tensors
        # h feeds nothing but this op, so the incoming gradient buffer is exclusively ours: transform it in place
        dh = H.f32c(dh)
        B, D2 = out.shape
        _call("mmvae_head_softmax_bwd", H.ptr(out), H.ptr(dh), B, D2 // 2, H.stream())
        return dh


def head_softmax(h):
    return HeadSoftmax.apply(h)


# ----------------------------------------------------------------------------------------------
# fused latent op
# ----------------------------------------------------------------------------------------------
_POE_TICKETS = {}      # device -> (zeroed int pool, {stream: slot}): the fusion backward's last-workgroup tickets


def _poe_ticket(dev):
    """device int owned by the current stream (two fusion backwards may run on different streams at once); the pool
    is allocated by the first call -- a warm-up pass -- so that a stream first seen during graph capture costs no
    allocation or memset node"""
    pool = _POE_TICKETS.get(dev.index)
    if pool is None:
        pool = _POE_TICKETS[dev.index] = (torch.zeros(64, dtype=torch.int32, device=dev), {})
    buf, slots = pool
    slot = slots.setdefault(H.stream(), len(slots))
    if slot >= buf.numel():
        return None           # more streams than slots: the two-launch path
    return buf.data_ptr() + 4 * slot


class PoeReparamKL(Function):
    """Product of experts -> n_z reparameterised samples -> analytic KL rows.

    packed[e]: (B, 2*Dtot) = [mu_e | lv_e] head outputs; the experts are columns [col0, col0+D) of both halves
    (col0 = 0, D = Dtot unless `cols` selects a sub-range: DMVAE's shared / private split).  Returns joint (2,B,D)
    [not differentiable], kl (E+1,B), then n_z tensors z_i (B,D)."""

    @staticmethod
    def forward(ctx, theta, gtheta, with_prior, n_z, kl_mask, E, cols, raw, rng, *tensors):
        """raw: the logvar halves of `packed` are the raw head outputs; softmax + 1e-6 happens inside the kernels.
        rng: None (the n_z noise tensors follow `packed`), or the device generator state: the kernel draws the noise"""
        packed = [H.f32c(t) for t in tensors[:E]]
        B, D2 = packed[0].shape
        if rng is not None:
            col_d = cols[1] if cols is not None else D2 // 2
            eps = list(torch.empty(n_z, B, col_d, device=packed[0].device).unbind(0))
        else:
            eps = [H.f32c(t) for t in tensors[E:E + n_z]]
        Dtot = D2 // 2
        col0, D = cols if cols is not None else (0, Dtot)
        dev = packed[0].device
        joint = torch.empty(2, B, D, device=dev)
        kl = torch.empty(E + 1, B, device=dev)
        zs = [torch.empty(B, D, device=dev) for _ in range(n_z)]     # separate tensors: no select/stack backward
        a = H.PoeFwdArgs()
        for e, p in enumerate(packed):
            a.mu[e] = p.data_ptr() + 4 * col0
            a.lv[e] = p.data_ptr() + 4 * (Dtot + col0)
        for i, t in enumerate(eps):
            a.eps[i] = t.data_ptr()
            a.z[i] = zs[i].data_ptr()
        _call("mmvae_poe_reparam_kl_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(joint), H.ptr(kl), E, int(with_prior),
              n_z, kl_mask, B, D, D2, int(bool(raw)), H.ptr(rng), H.stream())
        if cols is not None and not raw and GradReducer.share_packed_grads:
            for e, t in enumerate(packed):      # (backward: one gradient tensor per head output, handed over by its last reader)
                if ctx.needs_input_grad[9 + e]:
                    GradReducer.packed_uses[t.data_ptr()] = GradReducer.packed_uses.get(t.data_ptr(), 0) + 1
        ctx.save_for_backward(theta, *packed, *eps)
        ctx.n_eps_in = 0 if rng is not None else n_z
        ctx.cfg = (gtheta, with_prior, n_z, kl_mask, E, B, D, Dtot, col0, int(bool(raw)))
        ctx.mark_non_differentiable(joint)
        ctx.set_materialize_grads(False)
        return (joint, kl, *zs)

    @staticmethod
    def backward(ctx, _dj, dkl, *dzs):
        gtheta, with_prior, n_z, kl_mask, E, B, D, Dtot, col0, raw = ctx.cfg
        theta = ctx.saved_tensors[0]
        packed = ctx.saved_tensors[1:1 + E]
        eps = ctx.saved_tensors[1 + E:]
        dev = theta.device
        dkl = H.f32c(dkl) if dkl is not None else torch.zeros(E + 1, B, device=dev)
        dz = [H.f32c(g) if g is not None else torch.zeros(B, D, device=dev) for g in dzs] if n_z else None
        sub = D != Dtot
        acc_packed, ret_packed = 0, None
        if sub and not raw and GradReducer.share_packed_grads:
            # a head output whose column ranges are read by several fusion calls (DMVAE: joint, shared, private) gets ONE
            # gradient tensor per backward pass: the first call to run zero-fills it and hands it to autograd, the later ones
            # add their columns in place (mmvae_poe_reparam_kl_bwd_acc) and hand back nothing -- instead of a zero-filled
            # tensor per call and autograd's addition per extra call.  (All of them run on the fusion's stream, and the
            # head's own backward node waits for every consumer before it reads the tensor.)
            reg = GradReducer.packed_grads
            if not reg:      # (entries live for ONE backward pass: an address may belong to another tensor in the next)
                torch.autograd.Variable._execution_engine.queue_callback(GradReducer.packed_grads_done)
            fresh = [p for p in packed if p.data_ptr() not in reg]
            new = iter(torch.zeros(len(fresh), *fresh[0].shape, device=dev).unbind(0)) if fresh and all(
                p.shape == fresh[0].shape for p in fresh) else iter([torch.zeros_like(p) for p in fresh])
            dpacked, ret_packed = [], []
            for e, p in enumerate(packed):
                ent = reg.get(p.data_ptr())
                if ent is None:      # [tensor, calls still to come]: the forward pass counted this output's readers
                    ent = reg[p.data_ptr()] = [next(new), GradReducer.packed_uses.get(p.data_ptr(), 1)]
                else:
                    acc_packed |= 1 << e
                ent[1] -= 1
                # the LAST reader's backward hands the tensor to autograd: every addition is then queued in front of the
                # point at which the engine records the gradient as produced (the head's backward may run on another stream)
                ret_packed.append(ent[0] if ent[1] == 0 else None)
                dpacked.append(ent[0])
        elif sub and all(p.shape == packed[0].shape for p in packed):
            dpacked = list(torch.zeros(len(packed), *packed[0].shape, device=dev).unbind(0))     # ONE fill for all experts
        else:
            dpacked = [(torch.zeros_like(p) if sub else torch.empty_like(p)) for p in packed]
        a = H.PoeBwdArgs()
        for e, p in enumerate(packed):
            a.mu[e] = p.data_ptr() + 4 * col0
            a.lv[e] = p.data_ptr() + 4 * (Dtot + col0)
            a.dmu[e] = dpacked[e].data_ptr() + 4 * col0
            a.dlv[e] = dpacked[e].data_ptr() + 4 * (Dtot + col0)
        for i in range(n_z if dz is not None else 0):
            a.eps[i] = eps[i].data_ptr()
            a.dz[i] = dz[i].data_ptr()
        if gtheta is not None:
            dth, acc, ret = gtheta, 1, None
            GradReducer.writes(dev, gtheta)
        else:
            dth = ret = torch.empty_like(theta)
            acc = 0
        ws = H.workspace(H.lib().mmvae_poe_ws_floats(B, D), dev)
        _call("mmvae_poe_reparam_kl_bwd_acc", ctypes.byref(a), H.ptr(theta), H.ptr(dkl), H.ptr(dth), H.ptr(ws),
              _poe_ticket(dev), E,
              int(with_prior), n_z if dz is not None else 0, kl_mask, B, D, 2 * Dtot, raw, acc, acc_packed, H.stream())
        return (ret, None, None, None, None, None, None, None, None, *(dpacked if ret_packed is None else ret_packed),
                *([None] * ctx.n_eps_in))


class TcFusion(Function):
    """Product of experts (no prior expert) -> ONE reparameterised sample -> KL of the joint to the prior (row E) and to
    every expert (rows 0 .. E-1): MVTCAE's latent op (csrc/tcfusion.hip).  packed[e]: (B, 2 D) = [mu_e | lv_e] head
    outputs.  Returns joint (2,B,D) [not differentiable], kl (E+1,B), z (B,D)."""

    @staticmethod
    def forward(ctx, theta, gtheta, raw, eps, *packed):
        packed = [H.f32c(t) for t in packed]
        theta, eps = H.f32c(theta), H.f32c(eps)
        E = len(packed)
        B, D2 = packed[0].shape
        D = D2 // 2
        assert all(p.shape == (B, D2) for p in packed) and eps.shape == (B, D) and theta.numel() == D
        dev = packed[0].device
        joint = torch.empty(2, B, D, device=dev)
        kl = torch.empty(E + 1, B, device=dev)
        z = torch.empty(B, D, device=dev)
        a = H.TcFwdArgs()
        for e, p in enumerate(packed[:H.MAX_EXPERTS]):
            a.mu[e] = p.data_ptr()
            a.lv[e] = p.data_ptr() + 4 * D
        _call("mmvae_tc_fusion_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps), H.ptr(joint), H.ptr(kl), H.ptr(z), E, B, D,
              D2, int(bool(raw)), H.stream())
        ctx.save_for_backward(theta, eps, *packed)
        ctx.cfg = (gtheta, E, B, D, int(bool(raw)))
        ctx.mark_non_differentiable(joint)
        ctx.set_materialize_grads(False)
        return joint, kl, z

    @staticmethod
    def backward(ctx, _dj, dkl, dz):
        gtheta, E, B, D, raw = ctx.cfg
        theta, eps = ctx.saved_tensors[:2]
        packed = ctx.saved_tensors[2:]
        dev = theta.device
        # (an absent upstream gradient goes in as NULL: the kernel takes it as zeros)
        dkl = H.f32c(dkl) if dkl is not None else None
        dz = H.f32c(dz) if dz is not None else None
        dpacked = [torch.empty_like(p) for p in packed]
        a = H.TcBwdArgs()
        for e, p in enumerate(packed):
            a.mu[e] = p.data_ptr()
            a.lv[e] = p.data_ptr() + 4 * D
            a.dmu[e] = dpacked[e].data_ptr()
            a.dlv[e] = dpacked[e].data_ptr() + 4 * D
        if gtheta is not None:
            dth, acc, ret = gtheta, 1, None
            GradReducer.writes(dev, gtheta)
        elif ctx.needs_input_grad[0]:
            dth = ret = torch.empty_like(theta)
            acc = 0
        else:
            dth, acc, ret = None, 0, None
        ws = H.workspace(H.lib().mmvae_tc_fusion_ws_floats(B, D), dev)
        _call("mmvae_tc_fusion_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps), H.ptr(dz), H.ptr(dkl), H.ptr(dth),
              H.ptr(ws), E, B, D, 2 * D, raw, acc, H.stream())
        return (ret, None, None, None, *dpacked)


def tc_fusion(theta, packed, eps, gtheta=None, raw=False):
    """-> joint (2,B,D), kl (E+1,B), z (B,D) of the total-correlation fusion (TcFusion); gtheta: the prior parameter's
    preset gradient view, which the backward pass then adds to; raw: packed = [mu | raw logvar-head output]"""
    return TcFusion.apply(theta, gtheta, raw, eps, *packed)


class RowsFan(Function):
    """Latent samples -> the decoders' input batches in ONE launch, and every sample's gradient as ONE sum in backward
    (csrc/latent.hip: mmvae_rows_fan_fwd / _bwd).  plan = [(R, W, [(source index, row block r, first column c0), ...]), ...]:
    output o is (R * B, W), block (i, r, c0) writes source i (B, w_i) to rows [r * B, (r + 1) * B), columns [c0, c0 + w_i).
    Replaces torch.cat / repeat per decoder call and autograd's addition per extra consumer of a sample
    (POE.objective / DMVAE.objective; reference: models/mmvae_models.py:159-187, :494-502)."""

    @staticmethod
    def supported(plan, srcs):
        nb = sum(len(bl) for _, _, bl in plan)
        uses = [0] * len(srcs)
        for _, _, bl in plan:
            for i, _, _ in bl:
                uses[i] += 1
        return (nb <= H.FAN_MAX_BLOCKS and len(srcs) <= H.FAN_MAX_SRC and max(uses) <= H.FAN_MAX_USES and min(uses) >= 1
                and all(t.is_cuda and t.dim() == 2 and t.shape[0] == srcs[0].shape[0] for t in srcs))

    @staticmethod
    def forward(ctx, plan, *srcs):
        srcs = [H.f32c(t) for t in srcs]
        B, dev = srcs[0].shape[0], srcs[0].device
        outs = [torch.empty(R * B, W, device=dev) for R, W, _ in plan]
        t = H.FanBlocks()
        k = 0
        for (R, W, bl), out in zip(plan, outs):
            for i, r, c0 in bl:
                w = srcs[i].shape[1]
                assert 0 <= r < R and c0 + w <= W
                t.src[k], t.dst[k] = srcs[i].data_ptr(), out.data_ptr() + 4 * (r * B * W + c0)
                t.width[k], t.ld_src[k], t.ld_dst[k] = w, w, W
                k += 1
        t.n, t.B = k, B
        _call("mmvae_rows_fan_fwd", ctypes.byref(t), H.stream())
        ctx.plan, ctx.B, ctx.widths = plan, B, [t_.shape[1] for t_ in srcs]
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        plan, B, widths = ctx.plan, ctx.B, ctx.widths
        gs = [H.f32c(g) if g is not None else None for g in gs]
        dev = next(g.device for g in gs if g is not None)
        t = H.FanSum()
        outs, n = [None] * len(widths), 0
        slot = {}
        for (R, W, bl), g in zip(plan, gs):
            if g is None:
                continue
            for i, r, c0 in bl:
                if i not in slot:
                    slot[i] = n
                    outs[i] = torch.empty(B, widths[i], device=dev)
                    t.out[n], t.width[n], t.n_g[n] = outs[i].data_ptr(), widths[i], 0
                    n += 1
                s_, j = slot[i], t.n_g[slot[i]]
                t.g[s_][j], t.ld[s_][j] = g.data_ptr() + 4 * (r * B * W + c0), W
                t.n_g[s_] = j + 1
        t.n, t.B = n, B
        if n:
            _call("mmvae_rows_fan_bwd", ctypes.byref(t), H.stream())
        return (None, *outs)


def rows_fan(plan, srcs):
    """[output tensors] of RowsFan for `plan` over the source tensors `srcs` (see RowsFan)"""
    return list(RowsFan.apply(plan, *srcs))


class KlRow(Function):
    """row j of a fusion call's KL block (E + 1, B) as its own tensor's view.  Its backward hands the block's gradient back
    with ONLY row j written -- PoeReparamKL.backward reads the rows of its kl_mask and nothing else -- where autograd's select
    backward zero-fills the block first (a launch per KL term on the chain decoders -> fusion -> encoders)."""

    @staticmethod
    def forward(ctx, kl, j):
        ctx.shape, ctx.j = tuple(kl.shape), int(j)
        return kl[int(j)]

    @staticmethod
    def backward(ctx, g):
        out = torch.empty(ctx.shape, device=g.device, dtype=g.dtype)
        out[ctx.j].copy_(g)
        return out, None


def kl_row(kl, j):
    return KlRow.apply(kl, j)


class DecoderEnd(Function):
    """identity on a decoder's latent sample: its backward is the LAST node of that decoder's backward pass.  Parked
    tall-skinny weight gradients of the decoder (GradReducer.tw_park: fewer than eight are left) are launched here, on the
    decoder's stream and in front of the event the fusion's backward waits for -- the early optimiser launch folds and
    updates the decoders' range and must find every decoder gradient final."""

    @staticmethod
    def forward(ctx, z):
        return z.view_as(z)

    @staticmethod
    def backward(ctx, g):
        GradReducer.tw_flush_stream(torch.cuda.current_stream(g.device))
        return g


class EarlyStepPoint(Function):
    """identity on the packed head output of the tower that shares the fusion's stream: its backward is the first node
    that runs on that stream AFTER the fusion's backward has handed its gradients over (the engine records the events the
    other towers' streams wait for when PoeReparamKL.backward returns -- a launch queued inside that function would sit in
    front of them and hold the other tower's encoder backward up: measured, +9 us on both chains).  Every decoder's and the
    prior's gradient is final and stream-ordered in front of this point: it opens the way for GradReducer.run_early_step
    and queues the parked Linear weight gradients (GradReducer.flush_dw)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        GradReducer.early_ready = True   # (a weight-gradient launch on this stream IN FRONT of this point -- a decoder's --
                                         # must not trigger the early optimiser launch: the fusion's backward has not run)
        GradReducer.dw_open = False      # (the encoders' Linear layers behind this point keep their grouped launches)
        GradReducer.flush_dw()
        # the parked conv weight gradients' partials are written on the other stream: in front of the early optimiser launch
        # (here, not in front of that launch: an edge into the middle of the encoders' backward serialises the graph)
        done, GradReducer.cw_done = GradReducer.cw_done, None
        if done is not None:
            torch.cuda.current_stream(g.device).wait_event(done)
        return g


class StreamIdlePoint(Function):
    """identity on the latent sample of a decoder that does NOT share the fusion's stream: its backward is the last node of
    that decoder's backward pass, and its stream then idles until the fusion's backward has run on the other one (cfg2: the
    text decoder is done ~50 us before the image decoder).  GradReducer.side_head -- the FIRST half of the in-graph input
    ring's pull of the next batch over the host link -- is queued here; the second half stays behind the text encoder's last
    backward launch (GradReducer.side_tail)."""

    @staticmethod
    def forward(ctx, z):
        return z.view_as(z)

    @staticmethod
    def backward(ctx, g):
        fn, GradReducer.side_head = GradReducer.side_head, None
        if fn is not None:
            fn(g.device)
        return g


def poe_reparam_kl(theta, packed, eps, with_prior, kl_mask, gtheta=None, cols=None, raw=False, rng=None):
    """-> joint (2,B,D), kl (E+1,B), [z_0 .. z_{n_z-1}] each (B,D); cols = (col0, D) selects expert columns;
    raw: packed = [mu | raw logvar-head output] (VaeComponent.process_output(raw=True)).
    eps: the n_z noise tensors, or -- with rng = the device generator state (ops.randn) -- their NUMBER: the fusion
    kernel then draws them itself (same values as ops.randn((n_z, B, D), rng))"""
    assert not (raw and cols is not None), "raw heads: the softmax runs over the full head width"
    assert not (raw and int(with_prior) == 2), "raw heads: the pass-through posterior (with_prior = 2) takes lv as its scale"
    if rng is not None:
        out = PoeReparamKL.apply(theta, gtheta, with_prior, int(eps), kl_mask, len(packed), cols, raw, rng, *packed)
    else:
        out = PoeReparamKL.apply(theta, gtheta, with_prior, len(eps), kl_mask, len(packed), cols, raw, None, *packed,
                                 *eps)
    return out[0], out[1], list(out[2:])


# ----------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------
class BceRowsum(Function):
    """row[b] = sum_f bce(x_hat[b,f], t[b,f])   (ReconLoss.bce + .sum(-1), models/objectives.py:392-406)"""

    @staticmethod
    def forward(ctx, x_hat, target):
        x_hat, target = H.f32c(x_hat), H.f32c(target)
        B = x_hat.shape[0]
        F = x_hat.numel() // B
        row = torch.empty(B, device=x_hat.device)
        _call("mmvae_bce_rowsum_fwd", H.ptr(x_hat), H.ptr(target), H.ptr(row), B, F, B, H.stream())
        ctx.save_for_backward(x_hat, target)
        return row

    @staticmethod
    def backward(ctx, g):
        x_hat, target = ctx.saved_tensors
        B = x_hat.shape[0]
        F = x_hat.numel() // B
        dx = torch.empty_like(x_hat)
        _call("mmvae_bce_rowsum_bwd", H.ptr(x_hat), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(dx), B, F, H.stream())
        return dx, None


class BceElem(Function):
    """elementwise bce (B,F) -- the literal ReconLoss.bce output"""

    @staticmethod
    def forward(ctx, x_hat, target):
        x_hat, target = H.f32c(x_hat), H.f32c(target)
        out = torch.empty_like(x_hat)
        _call("mmvae_bce_elem_fwd", H.ptr(x_hat), H.ptr(target), H.ptr(out), x_hat.numel(), H.stream())
        ctx.save_for_backward(x_hat, target)
        return out

    @staticmethod
    def backward(ctx, g):
        x_hat, target = ctx.saved_tensors
        # d/dx = (x - t) / max(x (1 - x), 1e-12); tiny elementwise epilogue on the caller's grad
        return H.f32c(g) * (x_hat - target) / ((1 - x_hat) * x_hat).clamp_min(1e-12), None


class LprobRowsum(Function):
    """row[b] = sum_f -log p(target[b,f]) under Normal / Laplace(loc, scale); `scale` None = scale := loc (masked
    modalities).  ReconLoss.lprob summed per sample (models/objectives.py:409-424)."""

    @staticmethod
    def forward(ctx, loc, target, scale, laplace, perm_c=0, logit_grad=False):
        """laplace: bool, or (bit mask, block rows): rows [j, j+1) * block rows are Laplace where bit j is set.
        perm_c: loc is the (rows, perm_c, F / perm_c) NCHW output of a conv decoder paired with the target as if it
        had been permuted to (rows, F / perm_c, perm_c) (Dec_SVHN).  logit_grad: loc = sigmoid(logits) from the
        producing layer's epilogue; backward returns the gradient with respect to the logits."""
        loc, target = H.f32c(loc), H.f32c(target)
        lap, lap_rows = (int(laplace[0]), int(laplace[1])) if isinstance(laplace, tuple) else (int(laplace), 0)
        trows = target.shape[0]
        F_ = target.numel() // trows
        B = loc.numel() // F_            # rows of loc; > trows: K-sample output, target row = row % trows
        assert B * F_ == loc.numel() and B % trows == 0
        row = torch.empty(B, device=loc.device)
        sc = -1.0 if scale is None else float(scale)
        _call("mmvae_lprob_rowsum_fwd", H.ptr(loc), H.ptr(target), H.ptr(row), B, F_, trows, sc, lap, lap_rows,
              int(perm_c), H.stream())
        ctx.save_for_backward(loc, target)
        ctx.cfg = (sc, lap, lap_rows, B, F_, trows, int(perm_c), int(bool(logit_grad)))
        return row

    @staticmethod
    def backward(ctx, g):
        loc, target = ctx.saved_tensors
        sc, lap, lap_rows, B, F_, trows, perm_c, logit_grad = ctx.cfg
        d = torch.empty_like(loc)
        _call("mmvae_lprob_rowsum_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), B, F_, trows, sc, lap,
              lap_rows, perm_c, logit_grad, H.stream())
        return d, None, None, None, None, None


class OptimalSigmaRowsum(Function):
    """ReconLoss.optimal_sigma summed per sample (models/objectives.py:503-509): one log sigma per call."""

    @staticmethod
    def forward(ctx, loc, target):
        loc, target = H.f32c(loc), H.f32c(target)
        B = loc.shape[0]
        F_ = loc.numel() // B
        row = torch.empty(B, device=loc.device)
        stats = torch.empty(4, device=loc.device)
        ws = torch.empty(H.lib().mmvae_optimal_sigma_ws_floats(B, F_), device=loc.device)
        _call("mmvae_optimal_sigma_fwd", H.ptr(loc), H.ptr(target), H.ptr(row), H.ptr(stats), H.ptr(ws), B, F_,
              H.stream())
        ctx.save_for_backward(loc, target, stats)
        return row

    @staticmethod
    def backward(ctx, g):
        loc, target, stats = ctx.saved_tensors
        B = loc.shape[0]
        d = torch.empty_like(loc)
        _call("mmvae_optimal_sigma_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(stats), H.ptr(d), B,
              loc.numel() // B, H.stream())
        return d, None


class LprobElem(Function):
    """ReconLoss.lprob element-wise (models/objectives.py:409-424): -log p(target) under Normal / Laplace(loc, scale)
    as float64, NaN -> 0; `scale` None = scale := loc.  target may hold fewer (repeating) elements than loc."""

    @staticmethod
    def forward(ctx, loc, target, scale, laplace):
        loc, target = H.f32c(loc), H.f32c(target)
        out = torch.empty(loc.shape, dtype=torch.float64, device=loc.device)
        sc = -1.0 if scale is None else float(scale)
        _call("mmvae_lprob_elem_fwd", H.ptr(loc), H.ptr(target), H.ptr(out), loc.numel(), target.numel(), sc,
              int(bool(laplace)), H.stream())
        ctx.save_for_backward(loc, target)
        ctx.cfg = (sc, int(bool(laplace)))
        return out

    @staticmethod
    def backward(ctx, g):
        loc, target = ctx.saved_tensors
        g = g.to(torch.float64).contiguous()
        d = torch.empty_like(loc)
        _call("mmvae_lprob_elem_bwd", H.ptr(loc), H.ptr(target), H.ptr(g), H.ptr(d), loc.numel(), target.numel(),
              ctx.cfg[0], ctx.cfg[1], H.stream())
        return d, None, None, None


class OptimalSigmaElem(Function):
    """ReconLoss.optimal_sigma element-wise (models/objectives.py:503-509)"""

    @staticmethod
    def forward(ctx, loc, target):
        loc, target = H.f32c(loc), H.f32c(target)
        n = loc.numel()
        out = torch.empty_like(loc)
        stats = torch.empty(4, device=loc.device)
        ws = torch.empty(H.lib().mmvae_optimal_sigma_ws_floats(1, n), device=loc.device)
        _call("mmvae_optimal_sigma_elem_fwd", H.ptr(loc), H.ptr(target), H.ptr(out), H.ptr(stats), H.ptr(ws), n,
              H.stream())
        ctx.save_for_backward(loc, target, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        loc, target, stats = ctx.saved_tensors
        n = loc.numel()
        d = torch.empty_like(loc)
        ws = torch.empty(H.lib().mmvae_optimal_sigma_ws_floats(1, n), device=loc.device)
        _call("mmvae_optimal_sigma_elem_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(stats), H.ptr(ws),
              H.ptr(d), n, H.stream())
        return d, None


PW_L1, PW_MSE = 0, 1


class PointwiseRowsum(Function):
    """row[b] = sum_f |x - t| (kind PW_L1; ReconLoss.l1, objectives.py:427-442) or (x - t)^2 (PW_MSE; :444-459);
    target rows repeat (row b against target row b % target rows)"""

    @staticmethod
    def forward(ctx, x, target, kind):
        x, target = H.f32c(x), H.f32c(target)
        B = x.shape[0]
        F_ = x.numel() // B
        trows = target.numel() // F_
        assert trows * F_ == target.numel() and B % trows == 0
        row = torch.empty(B, device=x.device)
        _call("mmvae_pointwise_rowsum_fwd", H.ptr(x), H.ptr(target), H.ptr(row), B, F_, trows, int(kind), H.stream())
        ctx.save_for_backward(x, target)
        ctx.cfg = (B, F_, trows, int(kind))
        return row

    @staticmethod
    def backward(ctx, g):
        x, target = ctx.saved_tensors
        B, F_, trows, kind = ctx.cfg
        d = torch.empty_like(x)
        _call("mmvae_pointwise_rowsum_bwd", H.ptr(x), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), B, F_, trows, kind,
              H.stream())
        return d, None, None


class PointwiseElem(Function):
    """element-wise l1 / mse (the literal ReconLoss.l1 / .mse outputs)"""

    @staticmethod
    def forward(ctx, x, target, kind):
        x, target = H.f32c(x), H.f32c(target)
        out = torch.empty_like(x)
        _call("mmvae_pointwise_elem", H.ptr(x), H.ptr(target), None, H.ptr(out), x.numel(), int(kind), H.stream())
        ctx.save_for_backward(x, target)
        ctx.kind = int(kind)
        return out

    @staticmethod
    def backward(ctx, g):
        x, target = ctx.saved_tensors
        d = torch.empty_like(x)
        _call("mmvae_pointwise_elem", H.ptr(x), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), x.numel(), ctx.kind,
              H.stream())
        return d, None, None


def lprob_elem(loc, target, scale=0.75, laplace=False):
    return LprobElem.apply(loc, target, scale, laplace)


def optimal_sigma_elem(loc, target):
    return OptimalSigmaElem.apply(loc, target)


def pointwise_rowsum(x, target, kind):
    return PointwiseRowsum.apply(x, target, kind)


def pointwise_elem(x, target, kind):
    return PointwiseElem.apply(x, target, kind)


def lprob_rowsum(loc, target, scale=0.75, laplace=False, perm_c=0, logit_grad=False):
    return LprobRowsum.apply(loc, target, scale, laplace, perm_c, logit_grad)


def optimal_sigma_rowsum(loc, target):
    return OptimalSigmaRowsum.apply(loc, target)


class AddPEDropout(Function):
    """dropout(x + pe[t]) for x (T,B,D), pe (T,D); x None: the decoders' time queries dropout(pe[t]) broadcast"""

    @staticmethod
    def forward(ctx, x, pe, T, B, D, drop):
        y = torch.empty(T, B, D, device=pe.device)
        _call("mmvae_add_pe_dropout_fwd", H.ptr(H.f32c(x)) if x is not None else None, H.ptr(pe), H.ptr(y), T, B, D,
              _dp(drop, y.numel()), H.stream())
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dy = H.f32c(dy)
        dx = torch.empty_like(dy)
        _call("mmvae_dropout_act_bwd", H.ptr(dy), H.ptr(dy), H.ptr(dx), dy.numel(), H.ACT_NONE,
              ctx.drop.c() if ctx.drop is not None else None, H.stream())
        return dx, None, None, None, None, None


def add_pe_dropout(x, pe, T, B, D, drop=None):
    return AddPEDropout.apply(x, pe, T, B, D, drop)


# what one workgroup of ce_time_*_tile_kernel stages: CE_TILE / CE_TILE_V of csrc/loss.hip (the seeded launch exists for
# the tile kernel only)
CE_TILE, CE_TILE_V = 4096, 256


class CeOverTime(Function):
    """category_ce with the softmax over TIME (models/objectives.py:486-500): logits/target (B,T,V) ->
    loss (B,V) [per_v=True] or its row sums (B,)."""

    @staticmethod
    def forward(ctx, logits, target, per_v):
        logits, target = H.f32c(logits), H.f32c(target)
        B, T, V = logits.shape
        trows = target.shape[0]       # < B: K-sample logits, row r against target row r % trows (see BceSigmoidRowsum)
        assert tuple(target.shape[1:]) == (T, V) and B % trows == 0
        dev = logits.device
        loss = torch.empty(B, V, device=dev) if per_v else None
        row = None if per_v else torch.empty(B, device=dev)
        cs = ConstSeed.current
        ctx.seeded = None
        ctx.trows = trows
        if cs is not None and not per_v and logits.requires_grad and T * V <= CE_TILE and V <= CE_TILE_V and trows == B:
            dl = torch.empty_like(logits)
            _call("mmvae_ce_over_time_seeded", H.ptr(logits), H.ptr(target), H.ptr(row), cs.value, H.ptr(dl), B, T, V,
                  H.stream())
            ctx.seeded = (cs.seed.data_ptr(), dl)
        else:
            _call("mmvae_ce_over_time_fwd", H.ptr(logits), H.ptr(target), H.ptr(loss), H.ptr(row), B, T, V, trows,
                  H.stream())
        ctx.save_for_backward(logits, target)
        ctx.per_v = per_v
        return loss if per_v else row

    @staticmethod
    def backward(ctx, g):
        if ctx.seeded is not None and g.data_ptr() == ctx.seeded[0]:
            return ctx.seeded[1], None, None
        logits, target = ctx.saved_tensors
        B, T, V = logits.shape
        g = H.f32c(g)
        dl = torch.empty_like(logits)
        _call("mmvae_ce_over_time_bwd", H.ptr(logits), H.ptr(target), H.ptr(g) if ctx.per_v else None,
              None if ctx.per_v else H.ptr(g), H.ptr(dl), B, T, V, ctx.trows, H.stream())
        return dl, None, None


def _lincomb_fits(n, k):
    """the library refuses more rows / outputs than its weight table holds (MMVAE_ERR_UNSUPPORTED); the row-pointer
    table built here has the same size, so the refusal comes before it is filled"""
    if n > H.LC_MAX_ROWS or k > H.LC_MAX_OUT:
        raise RuntimeError(f"lincomb_rows: unsupported shape ({n} rows, {k} outputs; at most {H.LC_MAX_ROWS} and "
                           f"{H.LC_MAX_OUT})")


class LincombRows(Function):
    unit_seed_ptr = None      # data_ptr of the trainer's persistent backward seed (a ones scalar), see backward()

    """out_k = sum_n W[k][n] * sum_b rows_n[b]  -- ELBO assembly with host-side constant weights.
    `blocks`: tensors of shape (B,) or (r,B); their rows are addressed in place (no cat/stack kernel).  Returns the
    k outputs as k scalar tensors, so backward receives one upstream scalar per output (no select / fill kernels)."""

    @staticmethod
    def forward(ctx, W, *blocks):
        blocks = [H.f32c(t) for t in blocks]
        B = blocks[0].shape[-1]
        rows = [t.numel() // B for t in blocks]
        n, k = sum(rows), len(W)
        _lincomb_fits(n, k)
        rp = H.RowPtrs()
        i = 0
        for t, r in zip(blocks, rows):
            for j in range(r):
                rp.p[i] = t.data_ptr() + 4 * j * B
                i += 1
        flat = (H.c_f * (k * n))(*[float(x) for row in W for x in row])
        out = torch.empty(k, device=blocks[0].device)
        ctx.unit = None
        du = None
        if LincombRows.unit_seed_ptr is not None and any(t.requires_grad for t in blocks):
            # the trainer seeds backward with a persistent ones scalar: the row gradients are then constants, written
            # here, and backward() hands them out without a launch
            ctx.unit = [torch.empty(t.shape, device=t.device) for t in blocks]
            dp, i = H.RowPtrs(), 0
            for t, r in zip(ctx.unit, rows):
                for j in range(r):
                    dp.p[i] = t.data_ptr() + 4 * j * B
                    i += 1
            du = ctypes.byref(dp)
        _call("mmvae_lincomb_rowptrs_fwd", ctypes.byref(rp), flat, H.ptr(out), du, n, B, k, H.stream())
        ctx.cfg = (flat, n, B, k, rows, [tuple(t.shape) for t in blocks])
        ctx.keep = blocks
        ctx.set_materialize_grads(False)      # an unused output (kld is only logged) must not cost a zero-fill kernel
        return tuple(out.unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        flat, n, B, k, rows, shapes = ctx.cfg
        dev = ctx.keep[0].device
        if (ctx.unit is not None and gs[0] is not None and gs[0].data_ptr() == LincombRows.unit_seed_ptr
                and all(g is None for g in gs[1:])):
            return (None, *ctx.unit)
        gp = H.GPtrs()
        held = []
        for i, g in enumerate(gs):
            if g is not None:
                g = H.f32c(g)
                held.append(g)
                gp.g[i] = g.data_ptr()
        outs, dp, i = [], H.RowPtrs(), 0
        for r, shp in zip(rows, shapes):
            d = torch.empty(shp, device=dev)
            outs.append(d)
            for j in range(r):
                dp.p[i] = d.data_ptr() + 4 * j * B
                i += 1
        _call("mmvae_lincomb_rowptrs_bwd", ctypes.byref(gp), flat, ctypes.byref(dp), n, B, k, H.stream())
        return (None, *outs)


def lincomb_rows_args(blocks, W):
    """(row pointers, packed weights, out (k,), n, B, k) of lincomb_rows(blocks, W) without launching it (no autograd):
    for GradReducer.tail"""
    blocks = [H.f32c(t.detach()) for t in blocks]
    B = blocks[0].shape[-1]
    rows = [t.numel() // B for t in blocks]
    n, k = sum(rows), len(W)
    _lincomb_fits(n, k)
    rp = H.RowPtrs()
    i = 0
    for t, r in zip(blocks, rows):
        for j in range(r):
            rp.p[i] = t.data_ptr() + 4 * j * B
            i += 1
    flat = (H.c_f * (k * n))(*[float(x) for row in W for x in row])
    out = torch.empty(k, device=blocks[0].device)
    return {"args": (rp, flat, out, n, B, k), "keep": blocks, "done": False}


class SplitRows(Function):
    """(R * B, F) -> R row blocks (B, F) as views; backward is ONE concatenation of the blocks' gradients (autograd's own
    slice backward costs a zero-fill and a copy per block plus the additions)."""

    @staticmethod
    def forward(ctx, x, R):
        B = x.shape[0] // R
        ctx.R = R
        return tuple(x[k * B:(k + 1) * B] for k in range(R))

    @staticmethod
    def backward(ctx, *gs):
        ref = next(g for g in gs if g is not None)
        return torch.cat([g if g is not None else torch.zeros_like(ref) for g in gs], 0), None


def split_rows(x, R):
    return SplitRows.apply(x, R)


class NormalLogRatio(Function):
    """lw[b] = sum_d [log N(z; mu_r, s_r) - log N(z; mu_o, s_o)]; gradient only into packed_r (MoE, :56-62)"""

    @staticmethod
    def forward(ctx, packed_r, packed_o, z):
        packed_r, packed_o, z = H.f32c(packed_r), H.f32c(packed_o), H.f32c(z)
        B, D2 = packed_r.shape
        lw = torch.empty(B, device=z.device)
        _call("mmvae_normal_logratio_fwd", H.ptr(packed_r), H.ptr(packed_o), H.ptr(z), H.ptr(lw), B, D2 // 2,
              H.stream())
        ctx.save_for_backward(packed_r, z)
        return lw

    @staticmethod
    def backward(ctx, g):
        packed_r, z = ctx.saved_tensors
        B, D2 = packed_r.shape
        d = torch.empty_like(packed_r)
        _call("mmvae_normal_logratio_bwd", H.ptr(packed_r), H.ptr(z), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2,
              H.stream())
        return d, None, None


class ExpMul(Function):
    """exp(lw) * r"""

    @staticmethod
    def forward(ctx, lw, r):
        lw, r = H.f32c(lw), H.f32c(r)
        out = torch.empty_like(r)
        _call("mmvae_expmul_fwd", H.ptr(lw), H.ptr(r), H.ptr(out), r.numel(), H.stream())
        ctx.save_for_backward(lw, r)
        return out

    @staticmethod
    def backward(ctx, g):
        lw, r = ctx.saved_tensors
        dlw, dr = torch.empty_like(lw), torch.empty_like(r)
        _call("mmvae_expmul_bwd", H.ptr(lw), H.ptr(r), H.ptr(H.f32c(g)), H.ptr(dlw), H.ptr(dr), r.numel(), H.stream())
        return dlw, dr


class MoeElbo(Function):
    """loss = (sum_n W_n sum_b rows_n[b] + n_nz * beta * sum kld) / M  (see mmvae_moe_elbo_fwd); a row whose weighted
    sum is exactly 0 is dropped, as the reference's `lp.sum() != 0` filter does, and gets a zero gradient"""

    @staticmethod
    def forward(ctx, kld, W, beta, M, *rows):
        rows = [H.f32c(t) for t in rows]
        B, n = rows[0].shape[0], len(rows)
        V = torch.empty(n, B, device=rows[0].device)
        torch.stack(rows, out=V)
        kld = H.f32c(kld)
        flat = (H.c_f * n)(*[float(x) for x in W])
        out = torch.empty(2 + n, device=V.device)      # loss, n_nz, a keep flag per row
        _call("mmvae_moe_elbo_fwd", H.ptr(V), flat, H.ptr(kld), H.ptr(out), n, M, B, float(beta), H.stream())
        ctx.save_for_backward(out)
        ctx.cfg = (flat, n, M, B, float(beta), tuple(kld.shape))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        flat, n, M, B, beta, kshape = ctx.cfg
        drows = torch.empty(n, B, device=out.device)
        dkld = torch.empty(kshape, device=out.device)
        _call("mmvae_moe_elbo_bwd", H.ptr(H.f32c(g).reshape(1)), H.ptr(out), flat, H.ptr(drows), H.ptr(dkld), n, M, B,
              beta, H.stream())
        return (dkld, None, None, None, *[drows[i] for i in range(n)])


class LaplaceLogRatio(Function):
    """NormalLogRatio under Laplace posteriors (`prior: laplace`, models/mmvae_models.py:56-62)"""

    @staticmethod
    def forward(ctx, packed_r, packed_o, z):
        packed_r, packed_o, z = H.f32c(packed_r), H.f32c(packed_o), H.f32c(z)
        B, D2 = packed_r.shape
        lw = torch.empty(B, device=z.device)
        _call("mmvae_laplace_logratio_fwd", H.ptr(packed_r), H.ptr(packed_o), H.ptr(z), H.ptr(lw), B, D2 // 2,
              H.stream())
        ctx.save_for_backward(packed_r, z)
        return lw

    @staticmethod
    def backward(ctx, g):
        packed_r, z = ctx.saved_tensors
        B, D2 = packed_r.shape
        d = torch.empty_like(packed_r)
        _call("mmvae_laplace_logratio_bwd", H.ptr(packed_r), H.ptr(z), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2,
              H.stream())
        return d, None, None


class KlLaplaceNormal(Function):
    """kl[b] = sum_d KL(Laplace(mu, s) || N(0, 1)) for packed (B, 2D) = [mu | s]"""

    @staticmethod
    def forward(ctx, packed):
        packed = H.f32c(packed)
        B, D2 = packed.shape
        kl = torch.empty(B, device=packed.device)
        _call("mmvae_kl_laplace_normal_fwd", H.ptr(packed), H.ptr(kl), B, D2 // 2, H.stream())
        ctx.save_for_backward(packed)
        return kl

    @staticmethod
    def backward(ctx, g):
        (packed,) = ctx.saved_tensors
        B, D2 = packed.shape
        d = torch.empty_like(packed)
        _call("mmvae_kl_laplace_normal_bwd", H.ptr(packed), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2, H.stream())
        return d


class MoeKSample(Function):
    """K reparameterised samples per modality posterior + the latent part of the DReG importance weights
    (csrc/moe.hip; MOE.forward :96-100, _m_dreg_looser objectives.py:366-373).

    packed[m] (B,2D) = [mu | scale]; eps[m] (K,B,D) standard variates of q_m's family.  Returns lat (M,K,B) =
    sum_d log p(z) - log-mean-exp_m sum_d log q_m(z) and z (M,K,B,D) (one tensor: the decoders take all of it)."""

    @staticmethod
    def forward(ctx, theta, gtheta, laplace, M, beta, *tensors):
        packed = [H.f32c(t) for t in tensors[:M]]
        eps = [H.f32c(t) for t in tensors[M:2 * M]]
        K, B, D = eps[0].shape
        dev = packed[0].device
        z = torch.empty(M, K, B, D, device=dev)
        zs = z.unbind(0)
        lat = torch.empty(M, K, B, device=dev)
        pi = torch.empty(M, K, B, M, device=dev)
        a = H.MoeKArgs()
        for m in range(M):
            a.packed[m], a.eps[m], a.z[m], a.laplace[m] = packed[m].data_ptr(), eps[m].data_ptr(), zs[m].data_ptr(), \
                int(laplace[m])
        _call("mmvae_moe_ksample_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(lat), H.ptr(pi), M, K, B, D, float(beta),
              H.stream())
        ctx.save_for_backward(theta, pi, z, *packed, *eps)
        ctx.cfg = (gtheta, tuple(int(x) for x in laplace), M, K, B, D, float(beta))
        ctx.set_materialize_grads(False)
        return lat, z

    @staticmethod
    def backward(ctx, dlat, dz):
        gtheta, laplace, M, K, B, D, beta = ctx.cfg
        theta, pi, z = ctx.saved_tensors[:3]
        packed = ctx.saved_tensors[3:3 + M]
        eps = ctx.saved_tensors[3 + M:3 + 2 * M]
        zs = z.unbind(0)
        dev = theta.device
        dlat = H.f32c(dlat) if dlat is not None else torch.zeros(M, K, B, device=dev)
        dzs = list(H.f32c(dz).unbind(0)) if dz is not None else [None] * M
        dpacked = [torch.empty_like(p) for p in packed]
        a = H.MoeKBwdArgs()
        for m in range(M):
            a.packed[m], a.eps[m], a.z[m] = packed[m].data_ptr(), eps[m].data_ptr(), zs[m].data_ptr()
            a.dz[m] = dzs[m].data_ptr() if dzs[m] is not None else None
            a.dpacked[m], a.laplace[m] = dpacked[m].data_ptr(), laplace[m]
        ret = None
        rows = None
        if ctx.needs_input_grad[0] or gtheta is not None:
            rows = GradReducer.alloc(B * D, dev) if _defer(gtheta) else torch.empty(B, D, device=dev)
        _call("mmvae_moe_ksample_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(dlat), H.ptr(pi), H.ptr(rows), M, K, B, D,
              beta, H.stream())
        if rows is not None:
            if _defer(gtheta):
                GradReducer.add(rows.data_ptr(), gtheta, B, D, D)
            elif gtheta is not None:
                gtheta += rows.sum(0).view_as(gtheta)
            else:
                ret = rows.sum(0).view_as(theta)
        return (ret, None, None, None, None, *dpacked, *([None] * M))


def moe_ksample(theta, packed, eps, laplace, gtheta=None, beta=1.0):
    """-> lat (M,K,B) = log p(z) - beta log-mean-exp_m log q_m(z), z (M,K,B,D)"""
    return MoeKSample.apply(theta, gtheta, laplace, len(packed), beta, *packed, *eps)


class DregLoss(Function):
    """MultimodalObjective.dreg (objectives.py:375-387) from the latent terms `lat` (M,K,B) and the positive
    per-sample reconstruction sums own_r / cross_r (K*B): returns (loss fp64 scalar, lpx (M,2,K) fp64 [logged])."""

    @staticmethod
    def forward(ctx, lat, lam, M, *rows):
        lat = H.f32c(lat)
        rows = [H.f32c(r).reshape(-1) for r in rows]
        _, K, B = lat.shape
        assert len(rows) == 2 * M and all(r.numel() == K * B for r in rows)
        out = torch.empty(1 + 4 * M * K, dtype=torch.float64, device=lat.device)
        t = H.DregRows()
        for r in range(M):
            t.own[r], t.cross[r], t.lam[r] = rows[2 * r].data_ptr(), rows[2 * r + 1].data_ptr(), float(lam[r])
        _call("mmvae_dreg_loss_fwd", H.ptr(lat), ctypes.byref(t), H.ptr(out), M, K, B, H.stream())
        ctx.save_for_backward(out)
        ctx.cfg = (tuple(float(x) for x in lam), M, K, B, [tuple(r.shape) for r in rows])
        rec = out[1 + 2 * M * K:].view(M, 2, K)
        ctx.mark_non_differentiable(rec)
        return out[0], rec

    @staticmethod
    def backward(ctx, g, _grec):
        (out,) = ctx.saved_tensors
        lam, M, K, B, shapes = ctx.cfg
        dev = out.device
        g = g.to(torch.float64).reshape(1).contiguous()
        dlat = torch.empty(M, K, B, device=dev)
        drows = [torch.empty(K * B, device=dev) for _ in range(2 * M)]
        t = H.DregRows()
        for r in range(M):
            t.own[r], t.cross[r], t.lam[r] = drows[2 * r].data_ptr(), drows[2 * r + 1].data_ptr(), lam[r]
        _call("mmvae_dreg_loss_bwd", H.ptr(out), H.ptr(g), ctypes.byref(t), H.ptr(dlat), M, K, B, H.stream())
        return (dlat, None, None, *drows)


def dreg_loss(lat, lam, rows):
    return DregLoss.apply(lat, lam, len(lam), *rows)


class IwaeLoss(Function):
    """MultimodalObjective.iwae (objectives.py:342-359) from the latent terms `lat` (M,K,B) = log p(z) - beta lqz and
    the positive per-sample reconstruction sums own_r / cross_r (K*B): returns (loss fp64 scalar, lpx (M,2,K*B) fp64
    [logged]).  csrc/moe.hip: iwae_loss_*."""

    @staticmethod
    def forward(ctx, lat, lam, M, *rows):
        lat = H.f32c(lat)
        rows = [H.f32c(r).reshape(-1) for r in rows]
        _, K, B = lat.shape
        assert len(rows) == 2 * M and all(r.numel() == K * B for r in rows)
        out = torch.empty(H.lib().mmvae_iwae_loss_out_doubles(M, K, B), dtype=torch.float64, device=lat.device)
        t = H.DregRows()
        for r in range(M):
            t.own[r], t.cross[r], t.lam[r] = rows[2 * r].data_ptr(), rows[2 * r + 1].data_ptr(), float(lam[r])
        _call("mmvae_iwae_loss_fwd", H.ptr(lat), ctypes.byref(t), H.ptr(out), M, K, B, H.stream())
        ctx.save_for_backward(lat, out)
        ctx.cfg = (tuple(float(x) for x in lam), M, K, B)
        rec = out[1 + B:].view(M, 2, K * B)
        ctx.mark_non_differentiable(rec)
        return out[0], rec

    @staticmethod
    def backward(ctx, g, _grec):
        lat, out = ctx.saved_tensors
        lam, M, K, B = ctx.cfg
        dev = out.device
        g = g.to(torch.float64).reshape(1).contiguous()
        dlat = torch.empty(M, K, B, device=dev)
        drows = [torch.empty(K * B, device=dev) for _ in range(2 * M)]
        t = H.DregRows()
        for r in range(M):
            t.own[r], t.cross[r], t.lam[r] = drows[2 * r].data_ptr(), drows[2 * r + 1].data_ptr(), lam[r]
        _call("mmvae_iwae_loss_bwd", H.ptr(lat), H.ptr(out), H.ptr(g), ctypes.byref(t), H.ptr(dlat), M, K, B, H.stream())
        return (dlat, None, None, *drows)


def iwae_loss(lat, lam, rows):
    return IwaeLoss.apply(lat, lam, len(lam), *rows)


def normal_logratio(packed_r, packed_o, z):
    return NormalLogRatio.apply(packed_r, packed_o, z)


def laplace_logratio(packed_r, packed_o, z):
    return LaplaceLogRatio.apply(packed_r, packed_o, z)


def kl_laplace_normal(packed):
    return KlLaplaceNormal.apply(packed)


def expmul(lw, r):
    return ExpMul.apply(lw, r)


def moe_elbo(rows, W, kld, beta, M):
    return MoeElbo.apply(kld, W, beta, M, *rows)


def bce_rowsum(x_hat, target):
    return BceRowsum.apply(x_hat, target)


def bce_elem(x_hat, target):
    return BceElem.apply(x_hat, target)


def ce_over_time(logits, target, per_v=False):
    return CeOverTime.apply(logits, target, per_v)


def lincomb_rows(blocks, W):
    if torch.is_tensor(blocks):
        blocks = [blocks]
    return LincombRows.apply(W, *blocks)


# ----------------------------------------------------------------------------------------------
# text tower
# ----------------------------------------------------------------------------------------------
class EmbedPE(Function):
    """Embedding(one-hot.long()) + PositionalEncoding quirk -> (T, R * B0, 2V)  (models/encoders.py:833-835); R > 1: R passes
    over the same (B0, T, V) batch as one call, output row k * B0 + b (the repeat is never materialised)"""

    @staticmethod
    def forward(ctx, onehot, emb, pe, mode, gemb, drop, repeat=1):
        onehot = H.f32c(onehot)
        B0, T, V = onehot.shape
        B = B0 * repeat
        x = torch.empty(T, B, 2 * V, device=onehot.device)
        _call("mmvae_embed_pe_fwd", H.ptr(onehot), H.ptr(emb), H.ptr(pe), H.ptr(x), B, T, V, mode, B0, _dp(drop, x.numel()),
              H.stream())
        ctx.save_for_backward(onehot, emb)
        ctx.cfg = (mode, gemb, drop, repeat)
        return x

    @staticmethod
    def backward(ctx, dx):
        onehot, emb = ctx.saved_tensors
        mode, gemb, drop, repeat = ctx.cfg
        dpc = drop.c() if drop is not None else None
        B0, T, V = onehot.shape
        B = B0 * repeat
        dx = H.f32c(dx)
        de, acc, ret = _new_like_param(emb, gemb)
        nws = H.lib().mmvae_embed_ws_floats(B, T, V)
        if _defer(gemb):
            ws = GradReducer.alloc(nws, dx.device)
            _call("mmvae_embed_pe_bwd", H.ptr(onehot), H.ptr(dx), None, H.ptr(ws), B, T, V, mode, B0, H.ACC_DEFER, dpc,
                  H.stream())
            GradReducer.add(ws.data_ptr(), de, H.lib().mmvae_embed_bwd_rows(B, T, V), 4, 4)
        else:
            ws = H.workspace(nws, dx.device)
            _call("mmvae_embed_pe_bwd", H.ptr(onehot), H.ptr(dx), H.ptr(de), H.ptr(ws), B, T, V, mode, B0, acc, dpc,
                  H.stream())
        GradReducer.run_side_tail(dx.device)      # the text encoder's LAST backward launch: its stream idles from here on
        return None, ret, None, None, None, None, None


class Attention(Function):
    """softmax(q k^T / sqrt(hd) + key-padding mask) v for packed qkv (L, N, 3E), L <= 128, head_dim <= 32"""

    @staticmethod
    def forward(ctx, qkv, kpm, nhead, mask_is_valid, drop):
        qkv = H.f32c(qkv)
        L, N, E3 = qkv.shape
        E = E3 // 3
        hd = E // nhead
        out = torch.empty(L, N, E, device=qkv.device)
        probs = torch.empty(N, nhead, L, L, device=qkv.device)
        p = qkv.data_ptr()
        _call("mmvae_attn_fwd", p, p + 4 * E, p + 8 * E, H.ptr(kpm), H.ptr(out), H.ptr(probs), L, L, N, nhead, hd, E3,
              E3, E3, int(mask_is_valid), _dp(drop, probs.numel()), H.stream())
        ctx.save_for_backward(qkv, probs)
        ctx.nhead = nhead
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, probs = ctx.saved_tensors
        L, N, E3 = qkv.shape
        E = E3 // 3
        nhead = ctx.nhead
        dout = H.f32c(dout)
        dqkv = torch.empty_like(qkv)
        p, d = qkv.data_ptr(), dqkv.data_ptr()
        _call("mmvae_attn_bwd", p, p + 4 * E, p + 8 * E, H.ptr(probs), H.ptr(dout), d, d + 4 * E, d + 8 * E, L, L, N,
              nhead, E // nhead, E3, E3, E3, ctx.drop.c() if ctx.drop is not None else None, H.stream())
        return dqkv, None, None, None, None


def _linear_wgrad(dy2, x2, w, b, gw, gb, x_act=H.ACT_NONE):
    """dW (+)= dy2^T act(x2), db (+)= colsum(dy2) for dy2 (M,N), x2 (M,K): the weight half of Linear.backward.
    Returns the tensors to hand back to autograd (None when accumulated into the preset gradient views)."""
    M, N = dy2.shape
    K = x2.shape[1]
    dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, b is not None, N)
    nws = H.lib().mmvae_linear_bwd_weight_ws_floats(M, N, K)
    nz = H.lib().mmvae_linear_bwd_weight_splits(M, N, K)
    defer = _defer(gw, gb if b is not None else gw)
    if defer:
        ws = GradReducer.alloc(nws, dy2.device) if nz > 1 else None
        acc = H.ACC_DEFER
    else:
        ws, acc = H.workspace(nws, dy2.device), acc_w
    if gw is not None and not (defer and nz > 1):
        GradReducer.writes(dy2.device, gw, gb)
    _call("mmvae_linear_bwd_weight", H.ptr(dy2), H.ptr(x2), H.ptr(dw), H.ptr(db), H.ptr(ws), M, N, K, K, x_act, acc,
          H.stream())
    if defer and nz > 1:
        GradReducer.add(ws.data_ptr(), dw, nz, N * K, N * K)
        if db is not None:
            GradReducer.add(ws.data_ptr() + 4 * nz * N * K, db, nz, N, N)
    return ret_w, ret_b


# Round 4: ONE launch per fused text layer for all of its weight gradients on a kernel built for tall-skinny reductions
# (csrc/twgrad.hip: every operand row fetched once, 64 x 64 output units in registers, row slices over waves).
TXT_WGRAD = True      # (module switch for the tests: False = one launch per weight gradient)


def _txt_wgrad(jobs):
    """the weight half of every Linear behind a fused text layer: jobs = [(dy2, x2, w, b, gw, gb)] as _linear_wgrad takes them
    (round 2's mmvae_linear_bwd_weight_batch -- jobs on the split-K GEMM body in one grid -- now serves the parked Linear
    weight gradients: GradReducer.flush_dw)"""
    lib = H.lib()
    ok = TXT_WGRAD and 1 <= len(jobs) <= H.TXT_WGRAD_MAX and all(
        b is not None and _defer(gw, gb) and dy2.is_contiguous() and x2.is_contiguous() and
        lib.mmvae_txt_wgrad_supported(dy2.shape[0], dy2.shape[1], x2.shape[1]) for (dy2, x2, _, b, gw, gb) in jobs)
    if not ok:       # shapes the kernel does not take, or gradients handed back to autograd: one launch per job
        return [_linear_wgrad(*j) for j in jobs]
    arr = (H.TxtWgradJob * len(jobs))()
    segs = []
    for i, (dy2, x2, w, b, gw, gb) in enumerate(jobs):
        M, N = dy2.shape
        K = x2.shape[1]
        nz = lib.mmvae_txt_wgrad_splits(M, N, K)
        nws = lib.mmvae_txt_wgrad_ws_floats(M, N, K)
        ws = GradReducer.alloc(nws, dy2.device)
        j = arr[i]
        j.dy, j.x, j.ws, j.M, j.N, j.K = H.ptr(dy2), H.ptr(x2), H.ptr(ws), M, N, K
        segs.append((ws, nz, gw, gb, N, K, nws // nz))
    GradReducer.run_early_step(jobs[0][0].device)
    _call("mmvae_txt_wgrad", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())
    for ws, nz, gw, gb, N, K, pitch in segs:      # (partial row z: [N * K weight sums | N bias sums] at ws + z * pitch)
        GradReducer.add(ws.data_ptr(), gw, nz, N * K, pitch)
        GradReducer.add(ws.data_ptr() + 4 * N * K, gb, nz, N, pitch)
    return [(None, None)] * len(jobs)


class TxtLayerMeta:
    """static description of one fused transformer layer call (shapes + the DropSpecs of its dropout sites)"""

    def __init__(self, D, FF, NH, dec, drops, time_mean=False, heads=None):
        self.D, self.FF, self.NH, self.dec, self.drops = D, FF, NH, bool(dec), drops or {}
        self.time_mean = bool(time_mean)      # output (N, D): mean over the L frames (the encoder's pooling)
        # (w (HN, D), b (HN), gw, gb): the packed posterior heads applied to the pooled feature in the same launch;
        # gw / gb are the preset gradient views they accumulate into.  The output is then (N, HN).
        self.heads = heads
        assert heads is None or self.time_mean

    def c_drop(self, L, N):
        if not self.drops:
            return None
        t = H.TxtLayerDrop()
        n_el = {"attn": N * self.NH * L * L, "drop1": L * N * self.D, "xattn": N * self.NH * L, "drop2": L * N * self.D,
                "ffn": L * N * self.FF, "drop3": L * N * self.D}
        for k, n in n_el.items():
            d = self.drops.get(k)
            if d is not None:
                d.note(n)
                setattr(t, k, H.Dropout(d.state.data_ptr(), d.slot, d.site, d.p))
        return ctypes.byref(t)


_TXT_ENC_PARAMS = ("in_w", "in_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "n1_g", "n1_b", "n2_g", "n2_b")
_TXT_DEC_PARAMS = _TXT_ENC_PARAMS + ("n3_g", "n3_b", "x_in_w", "x_in_b", "x_out_w", "x_out_b")


def txt_layer_supported(L, D, FF, NH, dec):
    return bool(H.lib().mmvae_txt_layer_supported(int(L), int(D), int(FF), int(NH), int(bool(dec))))


class TxtLayer(Function):
    """One post-norm Transformer layer of the text towers in ONE launch per direction (csrc/txtlayer.hip):
    torch.nn.TransformerEncoderLayer, or TransformerDecoderLayer over a length-1 memory (`mem` (N,D))."""

    @staticmethod
    def forward(ctx, x, mem, mask_u8, meta, grads, *params):
        x = H.f32c(x)
        L, N, D = x.shape
        FF, NH, dec = meta.FF, meta.NH, meta.dec
        names = _TXT_DEC_PARAMS if dec else _TXT_ENC_PARAMS
        P = dict(zip(names, params))
        dev = x.device
        w = H.TxtLayerW()
        for k in names:
            setattr(w, k, P[k].data_ptr())
        if dec:
            mem = H.f32c(mem)
            w.x_in_w = P["x_in_w"].data_ptr() + 4 * 2 * D * D       # value rows of the cross in_proj
            w.x_in_b = P["x_in_b"].data_ptr() + 4 * 2 * D
        e = lambda *sh: torch.empty(*sh, device=dev)
        S = {"qkv": e(L, N, 3 * D), "ao": e(L, N, D), "xhat1": e(L, N, D), "rstd1": e(L, N), "x1": e(L, N, D),
             "h1": e(L, N, FF), "g": e(L, N, FF), "xhatf": e(L, N, D), "rstdf": e(L, N)}
        if dec:
            S.update({"vproj": e(N, D), "vb": e(L, N, D), "xhat2": e(L, N, D), "rstd2": e(L, N), "x2": e(L, N, D)})
        sv = H.TxtLayerSaved()
        for k, t in S.items():
            setattr(sv, k, t.data_ptr())
        y = e(N, D) if meta.time_mean else e(L, N, D)
        hw = hb = hout = None
        HN = 0
        if meta.heads is not None:
            hw, hb = meta.heads[0], meta.heads[1]
            HN = hw.shape[0]
            hout = e(N, HN)
            S["z"] = y
        _call("mmvae_txt_layer_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(mem) if dec else None, H.ptr(y), ctypes.byref(w),
              ctypes.byref(sv), meta.c_drop(L, N), L, N, D, FF, NH, int(dec), int(meta.time_mean), H.ptr(hw), H.ptr(hb),
              H.ptr(hout), HN, H.stream())
        ctx.meta, ctx.names, ctx.grads, ctx.S = meta, names, grads, S
        ctx.save_for_backward(x, mem if dec else None, mask_u8, *params)
        return y if hout is None else hout

    @staticmethod
    def backward(ctx, dy):
        x, mem, mask_u8, *params = ctx.saved_tensors
        meta, names, G, S = ctx.meta, ctx.names, ctx.grads, ctx.S
        L, N, D = x.shape
        FF, NH, dec = meta.FF, meta.NH, meta.dec
        P = dict(zip(names, params))
        dev = x.device
        dy = H.f32c(dy)
        if meta.heads is not None:     # heads first: dy (N, HN) -> dz (N, D), head gradients into their preset views
            hw, hb, hgw, hgb = meta.heads
            z = S["z"]
            HN = hw.shape[0]
            if dy.data_ptr() % 16:
                dy = dy.clone()
            dz = torch.empty(N, D, device=dev)
            lib = H.lib()
            nz = lib.mmvae_linear_bwd_splits(N, HN, D)
            nws = lib.mmvae_linear_bwd_ws_floats(N, HN, D)
            ws = GradReducer.alloc(nws, dev) if nz > 1 else None
            _call("mmvae_linear_bwd", H.ptr(dy), H.ptr(z), H.ptr(hw), None, H.ptr(dz), H.ptr(hgw), H.ptr(hgb),
                  H.ptr(ws), N, HN, D, D, H.ACT_NONE, H.EP_NONE, H.ACC_DEFER, H.stream())
            if nz > 1:
                GradReducer.add(ws.data_ptr(), hgw, nz, HN * D, HN * D)
                GradReducer.add(ws.data_ptr() + 4 * nz * HN * D, hgb, nz, HN, HN)
            dy = dz
        w = H.TxtLayerW()
        for k in names:
            setattr(w, k, P[k].data_ptr())
        if dec:
            w.x_in_w = P["x_in_w"].data_ptr() + 4 * 2 * D * D
            w.x_in_b = P["x_in_b"].data_ptr() + 4 * 2 * D
        sv = H.TxtLayerSaved()
        for k, t in S.items():
            if k != "z":
                setattr(sv, k, t.data_ptr())
        e = lambda *sh: torch.empty(*sh, device=dev)
        nln = 3 if dec else 2
        ln_names = [("n1_g", "n1_b"), ("n2_g", "n2_b")] + ([("n3_g", "n3_b")] if dec else [])
        ln_defer = all(_defer(G.get(g), G.get(b)) for g, b in ln_names)
        lnws = GradReducer.alloc(N * nln * 2 * D, dev) if ln_defer else e(N * nln * 2 * D)
        T = {"d_f": e(L, N, D), "d_h1": e(L, N, FF), "d_a": e(L, N, D), "d_qkv": e(L, N, 3 * D)}
        if dec:
            T.update({"d_ca": e(L, N, D), "d_v": e(N, D)})
        gr = H.TxtLayerGrads()
        for k, t in T.items():
            setattr(gr, k, t.data_ptr())
        gr.lnws = lnws.data_ptr()
        dx = e(L, N, D)
        dmem = e(N, D) if dec else None
        drops = meta.drops
        dstruct = None
        if drops:
            t = H.TxtLayerDrop()
            for k, d in drops.items():
                if d is not None:
                    setattr(t, k, H.Dropout(d.state.data_ptr(), d.slot, d.site, d.p))
            dstruct = ctypes.byref(t)
        _call("mmvae_txt_layer_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), H.ptr(dmem), ctypes.byref(w),
              ctypes.byref(sv), ctypes.byref(gr), dstruct, L, N, D, FF, NH, int(dec), int(meta.time_mean), H.stream())
        M = L * N
        ret = {}

        specs = [(T["d_qkv"].view(M, 3 * D), x.view(M, D), "in_w", "in_b", None),
                 (T["d_a"].view(M, D), S["ao"].view(M, D), "out_w", "out_b", None),
                 (T["d_h1"].view(M, FF), (S["x2"] if dec else S["x1"]).view(M, D), "l1_w", "l1_b", None),
                 (T["d_f"].view(M, D), S["g"].view(M, FF), "l2_w", "l2_b", None)]
        if dec:       # the cross attention over a length-1 memory only has value rows in its in_proj
            specs += [(T["d_ca"].view(M, D), S["vb"].view(M, D), "x_out_w", "x_out_b", None),
                      (T["d_v"], mem, "x_in_w", "x_in_b", slice(2 * D, 3 * D))]
        jobs = []
        for dyt, xt, wn, bn, wsl in specs:
            wt, bt, gw, gb = P[wn], P[bn], G.get(wn), G.get(bn)
            if wsl is not None:       # a row slice of the parameter
                wt, bt = wt[wsl], bt[wsl]
                gw = gw[wsl] if gw is not None else None
                gb = gb[wsl] if gb is not None else None
            jobs.append((dyt, xt, wt, bt, gw, gb))
        for (dyt, xt, wn, bn, wsl), (rw, rb) in zip(specs, _txt_wgrad(jobs)):
            if wsl is None:
                ret[wn], ret[bn] = rw, rb
            elif rw is not None:      # no preset gradient views: embed the slice gradient in a full-size zero tensor
                fw, fb = torch.zeros_like(P[wn]), torch.zeros_like(P[bn])
                fw[wsl], fb[wsl] = rw, rb
                ret[wn], ret[bn] = fw, fb
            else:
                ret[wn], ret[bn] = None, None
        if ln_defer:
            for k, (gn, bn) in enumerate(ln_names):
                GradReducer.add(lnws.data_ptr() + 4 * (k * 2 * D), G[gn], N, D, nln * 2 * D)
                GradReducer.add(lnws.data_ptr() + 4 * (k * 2 * D + D), G[bn], N, D, nln * 2 * D)
                ret[gn], ret[bn] = None, None
        else:
            sums = lnws.view(N, nln, 2, D).sum(0)
            for k, (gn, bn) in enumerate(ln_names):
                ret[gn], ret[bn] = sums[k, 0].contiguous(), sums[k, 1].contiguous()
        return (dx, dmem, None, None, None) + tuple(ret[k] for k in names)


def txt_layer(x, mem, mask_u8, meta, params, grads):
    names = _TXT_DEC_PARAMS if meta.dec else _TXT_ENC_PARAMS
    return TxtLayer.apply(x, mem, mask_u8, meta, grads, *[params[k] for k in names])


class LayerNormResidual(Function):
    """y = LayerNorm(x + r); r None, same shape, or (N,d) broadcast over the leading (time) axis"""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, gg, gb, drop, res_sink=None, proj=None, pre=None):
        """proj = (x_in, w, b): `x` is the placeholder output of a lazy Linear (ops.linear(..., lazy=True)) -- the product
        x_in w^T + b is computed here, in the same launch as the LayerNorm (d = 32: mmvae_proj32_ln_fwd)"""
        x = H.f32c(x)
        d = x.shape[-1]
        rows = x.numel() // d
        r_rows = 0
        if r is not None:
            r = H.f32c(r)
            if r.numel() != x.numel():
                r_rows = r.numel() // d
        y = torch.empty_like(x)
        xhat = torch.empty_like(x)
        rstd = torch.empty(rows, device=x.device)
        fused = False
        if pre is not None:      # (y, xhat, rstd) computed by the producer's launch (ops.ffn32(..., ln=...)): nothing to launch
            y, xhat, rstd = pre
            fused = True
        elif proj is not None:
            xin, pw, pb = proj
            xin = H.f32c(xin)
            al = lambda t: t.data_ptr() % 16 == 0
            fused = (d == 32 and xin.shape[-1] == 32 and r is not None and r_rows == 0 and pb is not None and pw.is_contiguous()
                     and all(al(t) for t in (xin, pw, pb, r, gamma, beta, y, xhat)))
            if fused:
                _call("mmvae_proj32_ln_fwd", H.ptr(xin), H.ptr(pw), H.ptr(pb), H.ptr(r), H.ptr(gamma), H.ptr(beta), H.ptr(y),
                      H.ptr(xhat), H.ptr(rstd), rows, _dp(drop, x.numel()), H.stream())
            else:      # the Linear after all (its output was never computed), then the plain LayerNorm below
                _call("mmvae_linear_fwd", H.ptr(xin), H.ptr(pw), H.ptr(pb), None, H.ptr(x), rows, d, xin.shape[-1],
                      xin.shape[-1], H.ACT_NONE, H.EP_NONE, H.stream())
        if not fused:
            _call("mmvae_layernorm_residual_fwd", H.ptr(x), H.ptr(r), H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(xhat),
                  H.ptr(rstd), rows, d, r_rows, _dp(drop, x.numel()), H.stream())
        ctx.save_for_backward(xhat, rstd, gamma)
        ctx.cfg = (gg, gb, r is not None, r_rows, tuple(x.shape), tuple(r.shape) if r is not None else None, drop)
        ctx.res_sink = res_sink if (r is not None and r_rows == 0) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, gamma = ctx.saved_tensors
        gg, gb, has_r, r_rows, xshape, rshape, drop = ctx.cfg
        dy = H.f32c(dy)
        d = xshape[-1]
        rows = xhat.numel() // d
        dsum = torch.empty_like(xhat)
        dxd = torch.empty_like(xhat) if drop is not None else None      # grad of x = dsum * mask under dropout
        dpc = drop.c() if drop is not None else None
        if gg is not None:
            dg, dbt, acc, ret_g, ret_b = gg, gb, 1, None, None
        else:
            both = torch.empty(2 * d, device=dy.device)
            dg, dbt, acc = both[:d], both[d:], 0
            ret_g, ret_b = dg, dbt
        nws = H.lib().mmvae_layernorm_ws_floats(rows, d)
        if _defer(gg, gb):
            ws = GradReducer.alloc(nws, dy.device)
            _call("mmvae_layernorm_residual_bwd", H.ptr(dy), H.ptr(xhat), H.ptr(rstd), H.ptr(gamma), H.ptr(dsum),
                  H.ptr(dxd), None, None, H.ptr(ws), rows, d, H.ACC_DEFER, dpc, H.stream())
            nb = H.lib().mmvae_layernorm_bwd_rows(rows, d)
            GradReducer.add(ws.data_ptr(), dg, nb, d, 2 * d)
            GradReducer.add(ws.data_ptr() + 4 * d, dbt, nb, d, 2 * d)
        else:
            ws = H.workspace(nws, dy.device)
            _call("mmvae_layernorm_residual_bwd", H.ptr(dy), H.ptr(xhat), H.ptr(rstd), H.ptr(gamma), H.ptr(dsum),
                  H.ptr(dxd), dg.data_ptr(), dbt.data_ptr(), H.ptr(ws), rows, d, acc, dpc, H.stream())
        dr = None
        if has_r and ctx.needs_input_grad[1]:
            if r_rows:
                dr = torch.empty(rshape, device=dy.device)
                _call("mmvae_sum_over_time", H.ptr(dsum), H.ptr(dr), rows // r_rows, r_rows, d, H.stream())
            elif ctx.res_sink is not None:
                ctx.res_sink.grad = dsum          # picked up by the sub-layer's first backward (ResidualGrad)
            else:
                dr = dsum
        dx = dxd if drop is not None else dsum
        return (dx if ctx.needs_input_grad[0] else None), dr, ret_g, ret_b, None, None, None, None, None, None


class MeanOverTime(Function):
    @staticmethod
    def forward(ctx, x):
        x = H.f32c(x)
        L, N, d = x.shape
        y = torch.empty(N, d, device=x.device)
        _call("mmvae_mean_over_time_fwd", H.ptr(x), H.ptr(y), L, N, d, H.stream())
        ctx.shape = (L, N, d)
        return y

    @staticmethod
    def backward(ctx, dy):
        L, N, d = ctx.shape
        dy = H.f32c(dy)
        dx = torch.empty(L, N, d, device=dy.device)
        _call("mmvae_mean_over_time_bwd", H.ptr(dy), H.ptr(dx), L, N, d, H.stream())
        return dx


class PermuteMask(Function):
    """(T,B,V) -> (B,T,V) * mask[b,t]   (models/decoders.py:722); keep = Tk: the first Tk steps only, (B,Tk,V) -- the slice
    BaseObjective.recon_loss_fn takes afterwards (objectives.py:30-52) folded into the launch, zeros beyond Tk in backward"""

    @staticmethod
    def forward(ctx, x, mask_u8, keep=None):
        x = H.f32c(x)
        T, B, V = x.shape
        Tk = T if keep is None else int(keep)
        assert 0 < Tk <= T and tuple(mask_u8.shape) == (B, T)
        y = torch.empty(B, Tk, V, device=x.device)
        if Tk == T:
            _call("mmvae_permute_mask_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(y), T, B, V, H.stream())
        else:
            _call("mmvae_permute_mask_head_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(y), T, B, V, Tk, H.stream())
        ctx.save_for_backward(mask_u8)
        ctx.shape = (T, B, V, Tk)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask_u8,) = ctx.saved_tensors
        T, B, V, Tk = ctx.shape
        dy = H.f32c(dy)
        dx = torch.empty(T, B, V, device=dy.device)
        if Tk == T:
            _call("mmvae_permute_mask_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), T, B, V, H.stream())
        else:
            _call("mmvae_permute_mask_head_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), T, B, V, Tk, H.stream())
        return dx, None, None


def embed_pe(onehot, emb, pe, mode, gemb=None, drop=None, repeat=1):
    return EmbedPE.apply(onehot, emb, pe, mode, gemb, drop, repeat)


def attention(qkv, mask_u8, nhead, mask_is_valid=False, drop=None):
    """mask_u8 (N,L) bytes: key-padding mask (1 = ignore) or, with mask_is_valid, the validity mask (1 = token)"""
    return Attention.apply(qkv, mask_u8, nhead, mask_is_valid, drop)


def as_u8(mask):
    """zero-copy byte view of a bool mask (torch.bool is one 0/1 byte per element)"""
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    return mask.to(torch.uint8).contiguous()


def layernorm_residual(x, r, gamma, beta, gg=None, gb=None, drop=None, res_sink=None):
    """LayerNorm(dropout(x) + r); res_sink: the ResidualGrad that the op producing x from r also holds.  An x that is the
    placeholder of a lazy Linear (x._proj) has its product computed in the LayerNorm's launch"""
    return LayerNormResidual.apply(x, r, gamma, beta, gg, gb, drop, res_sink, getattr(x, "_proj", None),
                                   getattr(x, "_ln_pre", None))


class DropoutAct(Function):
    """y = dropout(act(x)), act in {none, gelu}"""

    @staticmethod
    def forward(ctx, x, act, drop):
        x = H.f32c(x)
        y = torch.empty_like(x)
        _call("mmvae_dropout_act_fwd", H.ptr(x), H.ptr(y), x.numel(), act, _dp(drop, x.numel()), H.stream())
        ctx.save_for_backward(x)
        ctx.cfg = (act, drop)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        act, drop = ctx.cfg
        dy = H.f32c(dy)
        dx = torch.empty_like(x)
        _call("mmvae_dropout_act_bwd", H.ptr(dy), H.ptr(x), H.ptr(dx), x.numel(), act, drop.c() if drop else None,
              H.stream())
        return dx, None, None


class HeadBcastDropout(Function):
    """(N,E) -> (L,N,E) with per-(n, head, l) attention-weight dropout (length-1 memory cross-attention)"""

    @staticmethod
    def forward(ctx, v, L, nhead, drop):
        v = H.f32c(v)
        N, E = v.shape
        out = torch.empty(L, N, E, device=v.device)
        _call("mmvae_head_bcast_dropout_fwd", H.ptr(v), H.ptr(out), L, N, nhead, E // nhead, _dp(drop, N * nhead * L),
              H.stream())
        ctx.cfg = (L, N, E, nhead, drop)
        return out

    @staticmethod
    def backward(ctx, dout):
        L, N, E, nhead, drop = ctx.cfg
        dout = H.f32c(dout)
        dv = torch.empty(N, E, device=dout.device)
        _call("mmvae_head_bcast_dropout_bwd", H.ptr(dout), H.ptr(dv), L, N, nhead, E // nhead,
              drop.c() if drop else None, H.stream())
        return dv, None, None, None


class Ffn32(Function):
    """linear2(dropout(gelu(linear1(x)))) of a post-norm Transformer layer with d_model = 32, fused (csrc/ffn.hip): the
    (rows, FF) hidden activation stays in registers, backward recomputes it.  x (..., 32); w1 (FF,32), b1 (FF),
    w2 (32,FF), b2 (32); drop: DropSpec of the hidden dropout or None; g*: the parameters' flat gradient views."""

    last_pre = None      # (y, xhat, rstd) of the LayerNorm epilogue of the forward that just ran (ops.ffn32 takes it)

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, drop, gw1, gb1, gw2, gb2, wsplit=None, res_sink=None, ln=None):
        """ln = (r, gamma, beta, ln_drop): the LayerNorm that consumes the block runs as this launch's epilogue (split-bf16
        path; mmvae_ffn32_fwd_b16_ln): the returned tensor is then a PLACEHOLDER carrying `_ln_pre = (y, xhat, rstd)`, which
        ops.layernorm_residual picks up instead of launching"""
        ctx.res_sink = res_sink
        x = H.f32c(x)
        M, FF = x.numel() // 32, w1.shape[0]
        y = torch.empty_like(x)
        if not FFN32_SPLIT_BF16:
            wsplit = None
        if FFN32_SPLIT_BF16:
            # the weights' three-term bf16 image, shared by the three launches (csrc/ffn_b16.inc): the caller's (one launch
            # for all layers of a tower: ffn32_prep_many), else made here
            if wsplit is None:
                wsplit = torch.empty(H.lib().mmvae_ffn32_wsplit_bytes(FF), dtype=torch.uint8, device=x.device)
                _call("mmvae_ffn32_prep_weights", H.ptr(w1), H.ptr(w2), H.ptr(wsplit), FF, H.stream())
            if ln is not None:
                r_, gamma_, beta_, ln_drop = ln
                r_ = H.f32c(r_)
                yln, xhat, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(M, device=x.device)
                _call("mmvae_ffn32_fwd_b16_ln", H.ptr(x), H.ptr(wsplit), H.ptr(b1), H.ptr(b2), H.ptr(r_), H.ptr(gamma_),
                      H.ptr(beta_), H.ptr(yln), H.ptr(xhat), H.ptr(rstd), M, FF, _dp(drop, M * FF), _dp(ln_drop, M * 32),
                      H.stream())
                Ffn32.last_pre = (yln, xhat, rstd)
            else:
                _call("mmvae_ffn32_fwd_b16", H.ptr(x), H.ptr(wsplit), H.ptr(b1), H.ptr(b2), H.ptr(y), M, FF,
                      _dp(drop, M * FF), H.stream())
        else:
            _call("mmvae_ffn32_fwd", H.ptr(x), H.ptr(w1), H.ptr(b1), H.ptr(w2), H.ptr(b2), H.ptr(y), M, FF,
                  _dp(drop, M * FF), H.stream())
        ctx.save_for_backward(x, w1, b1, w2)
        ctx.wsplit = wsplit
        ctx.cfg = (drop, gw1, gb1, gw2, gb2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, b1, w2 = ctx.saved_tensors
        drop, gw1, gb1, gw2, gb2 = ctx.cfg
        dy = H.f32c(dy)
        M, FF = x.numel() // 32, w1.shape[0]
        lib = H.lib()
        parts, rowlen = lib.mmvae_ffn32_bwd_parts(M, FF), lib.mmvae_ffn32_bwd_rowlen(FF)
        defer = _defer(gw1, gb1, gw2, gb2)
        ws = GradReducer.alloc(parts * rowlen, x.device) if defer else torch.empty(parts * rowlen, device=x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dc = drop.c() if drop else None
        other = StreamPlan.other_stream(x.device) if (dx is not None and defer and M * FF >= (1 << 20)
                                                      and FFN32_WGRAD_OTHER_STREAM) else None
        wsplit = ctx.wsplit
        radd = ctx.res_sink.take() if ctx.res_sink is not None else None      # the residual branch's gradient of x
        if dx is None:
            radd = None
        kadd = None                                                            # ... added by the data-gradient kernel
        if wsplit is not None:
            rsplit = torch.empty(lib.mmvae_ffn32_rsplit_bytes(M), dtype=torch.uint8, device=x.device)
            if radd is not None and radd.is_contiguous() and radd.numel() == x.numel():
                kadd, radd = radd, None

            def bwd(dx_, ws_):
                _call("mmvae_ffn32_bwd_b16", H.ptr(x), H.ptr(dy), H.ptr(wsplit), H.ptr(b1), H.ptr(dx_), H.ptr(ws_), H.ptr(rsplit),
                      H.ptr(kadd) if dx_ is not None else None, M, FF, dc, H.stream())
        else:
            rsplit = None

            def bwd(dx_, ws_):
                _call("mmvae_ffn32_bwd", H.ptr(x), H.ptr(dy), H.ptr(w1), H.ptr(b1), H.ptr(w2),
                      H.ptr(dx_) if dx_ is not None else None, H.ptr(ws_) if ws_ is not None else None, M, FF, dc, H.stream())
        if other is not None:
            # the weight-gradient launch (nothing but the end-of-backward fold reads it) goes to the step's OTHER stream,
            # which idles while a long tower's chain runs on this one; only dy and x have to exist, not the data gradient
            cur = torch.cuda.current_stream(x.device)
            ev = torch.cuda.Event()
            ev.record(cur)
            bwd(dx, None)
            other.wait_event(ev)
            with torch.cuda.stream(other):
                bwd(None, ws)
            held = (x, dy) if wsplit is None else (x, dy, wsplit, rsplit)
            for t in held:
                t.record_stream(other)
            GradReducer.keep(x.device, *held)
            GradReducer.note_stream(x.device, other)
        else:
            bwd(dx, ws)
        offs = (0, 32 * FF, 32 * FF + FF, 64 * FF + FF)
        lens = (32 * FF, FF, 32 * FF, 32)
        rets = [None, None, None, None]
        if defer:
            for o, ln, g in zip(offs, lens, (gw1, gb1, gw2, gb2)):
                GradReducer.add(ws.data_ptr() + 4 * o, g, parts, ln, rowlen)
        else:
            for i, (o, ln, g, like) in enumerate(zip(offs, lens, (gw1, gb1, gw2, gb2), (w1, b1, w2, b1[:32]))):
                dst, acc, ret = _new_like_param(like, g)
                _call("mmvae_reduce_rows", H.ptr(ws) + 4 * o, H.ptr(dst), parts, ln, rowlen, acc, H.stream())
                rets[i] = ret
        if radd is not None and dx is not None:
            dx = dx + radd.view_as(dx)
        return (dx, *rets, None, None, None, None, None, None, None, None)


# the fused feed-forward launches on split-bf16 MFMA (csrc/ffn_b16.inc) instead of fp32 MFMA (csrc/ffn.hip); both are tested
FFN32_SPLIT_BF16 = True
# large feed-forward weight-gradient launches go to the step's other stream (nothing but the end-of-backward fold reads them)
FFN32_WGRAD_OTHER_STREAM = True


def ffn32_supported(d, ff):
    return bool(H.lib().mmvae_ffn32_supported(int(d), int(ff)))


FFN32_LN = os.environ.get("MMVAE_FFN32_LN", "1") == "1"      # the LayerNorm behind the block as the forward launch's epilogue


def ffn32(x, w1, b1, w2, b2, drop=None, wsplit=None, res_sink=None, ln=None):
    """ln = (r, gamma, beta, ln_drop) of the LayerNorm(dropout(.) + r) that consumes the result: computed in the same launch
    when the split-bf16 core runs (the result is then a placeholder for ops.layernorm_residual, see Ffn32.forward)"""
    fuse = (ln is not None and FFN32_LN and FFN32_SPLIT_BF16 and x.is_cuda and ln[0].numel() == x.numel()
            and ln[0].is_contiguous() and ln[0].dtype == torch.float32)
    y = Ffn32.apply(x, w1, b1, w2, b2, drop, w1.grad, b1.grad, w2.grad, b2.grad, wsplit, res_sink, ln if fuse else None)
    if fuse:
        y._ln_pre, Ffn32.last_pre = Ffn32.last_pre, None
    return y


def ffn32_prep_many(pairs):
    """split-bf16 weight images of several feed-forward blocks [(w1, w2), ...] (same FF, <= 16) in ONE launch; returns one
    uint8 tensor per block for `ffn32(..., wsplit=)`.  None when the fp32 core is selected."""
    if not FFN32_SPLIT_BF16 or not pairs:
        return None
    FF, n, dev = pairs[0][0].shape[0], len(pairs), pairs[0][0].device
    nb = H.lib().mmvae_ffn32_wsplit_bytes(FF)
    buf = torch.empty(n, nb, dtype=torch.uint8, device=dev)
    arr = ctypes.c_void_p * n
    _call("mmvae_ffn32_prep_weights_many", arr(*[w1.data_ptr() for w1, _ in pairs]), arr(*[w2.data_ptr() for _, w2 in pairs]),
          arr(*[buf[i].data_ptr() for i in range(n)]), n, FF, H.stream())
    return [buf[i] for i in range(n)]


def dropout_act(x, act, drop):
    return DropoutAct.apply(x, act, drop)


def head_bcast_dropout(v, L, nhead, drop):
    return HeadBcastDropout.apply(v, L, nhead, drop)


def mean_over_time(x):
    return MeanOverTime.apply(x)


def permute_mask(x, mask_u8, keep=None):
    return PermuteMask.apply(x, mask_u8, keep)


# ----------------------------------------------------------------------------------------------
# optimiser / utilities (no autograd)
# ----------------------------------------------------------------------------------------------
# ----------------------------------------------------------------------------------------------
# Enc_TxtRNN: embedding-folded bidirectional GRU, last position only (csrc/gru.hip)
# ----------------------------------------------------------------------------------------------
def gru_token_ids(onehot):
    """(B,T,V) one-hot -> ids (T,B) int32 [argmax; padding rows = token 0], canonical one-hot rows (T*B, V)"""
    onehot = H.f32c(onehot)
    B, T, V = onehot.shape
    ids = torch.empty(T, B, dtype=torch.int32, device=onehot.device)
    oh = torch.empty(T * B, V, device=onehot.device)
    _call("mmvae_gru_token_ids", H.ptr(onehot), H.ptr(ids), H.ptr(oh), B, T, V, H.stream())
    return ids, oh


class GruForward(Function):
    """h_T of a one-layer GRU over T steps from h_0 = 0 (torch.nn.GRU's equations, gate order r, z, n), the input
    projection given as the embedding-folded table pt (3H,V) = W_ih E^T: gx_t = pt[:, id_t] + b_ih.
    Backward: T steps of gate derivatives + dh_{t-1} += dGh W_hh, then d W_hh / d b_hh and d pt / d b_ih as two
    (T B)-row reductions on the MFMA weight-gradient kernels."""

    @staticmethod
    def forward(ctx, pt, b_ih, w_hh, b_hh, ids, oh, gw_hh, gb_hh):
        pt, b_ih, w_hh, b_hh = H.f32c(pt), H.f32c(b_ih), H.f32c(w_hh), H.f32c(b_hh)
        T, B = ids.shape
        Hd, V = w_hh.shape[1], pt.shape[1]
        dev = pt.device
        hs = torch.empty(T + 1, B, Hd, device=dev)
        fill(hs[0], 0.0)
        saved = torch.empty(4, T, B, Hd, device=dev)
        _call("mmvae_gru_forward", H.ptr(pt), H.ptr(b_ih), H.ptr(w_hh), H.ptr(b_hh), H.ptr(ids), H.ptr(hs), H.ptr(saved),
              T, B, Hd, V, H.stream())
        ctx.save_for_backward(pt, b_ih, w_hh, b_hh, hs, saved, oh)
        ctx.cfg = (T, B, Hd, V, gw_hh, gb_hh)
        return hs[T]

    @staticmethod
    def backward(ctx, dhT):
        pt, b_ih, w_hh, b_hh, hs, saved, oh = ctx.saved_tensors
        T, B, Hd, V, gw_hh, gb_hh = ctx.cfg
        dev = pt.device
        dh = H.f32c(dhT).clone()
        dgx = torch.empty(T, B, 3 * Hd, device=dev)
        dgh = torch.empty(T, B, 3 * Hd, device=dev)
        _call("mmvae_gru_backward", H.ptr(dh), H.ptr(w_hh), H.ptr(hs), H.ptr(saved), H.ptr(dgx), H.ptr(dgh), T, B, Hd,
              H.stream())
        # d W_hh (3H,H) = sum_t dGh_t^T h_{t-1}, d b_hh = column sums: reduction over the T*B rows
        ret_whh, ret_bhh = _linear_wgrad(dgh.view(T * B, 3 * Hd), hs[:T].reshape(T * B, Hd), w_hh, b_hh, gw_hh, gb_hh)
        # d pt (3H,V) = sum_t dGx_t^T onehot(id_t), d b_ih = column sums
        d_pt, d_bih = _linear_wgrad(dgx.view(T * B, 3 * Hd), oh, pt, b_ih, None, None)
        return d_pt, d_bih, ret_whh, ret_bhh, None, None, None, None


class GruCell0(Function):
    """out = h_fwd + GRU cell step from h = 0 on the last token (the reverse direction at the last position)"""

    @staticmethod
    def forward(ctx, pt, b_ih, b_hh, ids_last, oh_last, h_fwd, w_hh_shape):
        pt, b_ih, b_hh, h_fwd = H.f32c(pt), H.f32c(b_ih), H.f32c(b_hh), H.f32c(h_fwd)
        B, Hd = h_fwd.shape
        V = pt.shape[1]
        out = torch.empty_like(h_fwd)
        saved = torch.empty(3, B, Hd, device=pt.device)
        _call("mmvae_gru_cell0_fwd", H.ptr(pt), H.ptr(b_ih), H.ptr(b_hh), H.ptr(ids_last), H.ptr(h_fwd), H.ptr(out),
              H.ptr(saved), B, Hd, V, H.stream())
        ctx.save_for_backward(pt, b_ih, b_hh, saved, oh_last)
        ctx.cfg = (B, Hd, V)
        return out

    @staticmethod
    def backward(ctx, dout):
        pt, b_ih, b_hh, saved, oh_last = ctx.saved_tensors
        B, Hd, V = ctx.cfg
        dout = H.f32c(dout)
        dgx = torch.empty(B, 3 * Hd, device=pt.device)
        dgh = torch.empty(B, 3 * Hd, device=pt.device)
        _call("mmvae_gru_cell0_bwd", H.ptr(dout), H.ptr(saved), H.ptr(b_hh), H.ptr(dgx), H.ptr(dgh), B, Hd, H.stream())
        d_pt, d_bih = _linear_wgrad(dgx, oh_last, pt, b_ih, None, None)
        _, d_bhh = _linear_wgrad(dgh, oh_last, pt, b_hh, None, None)      # column sums of dGh (the dW half is unused)
        return d_pt, d_bih, d_bhh, None, None, dout, None


def gru_forward(pt, b_ih, w_hh, b_hh, ids, oh, gw_hh=None, gb_hh=None):
    return GruForward.apply(pt, b_ih, w_hh, b_hh, ids, oh, gw_hh, gb_hh)


def gru_cell0(pt, b_ih, b_hh, ids_last, oh_last, h_fwd):
    return GruCell0.apply(pt, b_ih, b_hh, ids_last, oh_last, h_fwd, None)


WEIGHT_GEN = [0]      # bumped by every optimiser launch: caches derived from the weights (split-bf16 images) carry it


def adam_amsgrad_flat(p, g, m, v, vmax, lr, beta1, beta2, eps, step, step_dev=None, grad_scale=1.0, zero_grad=True):
    WEIGHT_GEN[0] += 1
    _call("mmvae_adam_amsgrad_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), lr, beta1, beta2,
          eps, int(step), H.ptr(step_dev), grad_scale, int(zero_grad), H.stream())


def adabelief_flat(p, g, m, s, lr, beta1, beta2, eps, step, step_dev=None, grad_scale=1.0, zero_grad=True):
    WEIGHT_GEN[0] += 1
    _call("mmvae_adabelief_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(s), p.numel(), lr, beta1, beta2, eps, int(step),
          H.ptr(step_dev), grad_scale, int(zero_grad), H.stream())


def _tail_args(tail):
    """the ELBO assembly that rides on a fold + Adam launch (GradReducer.tail) as that launch's trailing arguments"""
    if tail is None:
        return None, None, None, 0, 0, 0
    rp, flat, out, n, B, k = tail["args"]
    return ctypes.byref(rp), flat, H.ptr(out), n, B, k


def adam_fold_flat(p, g, m, v, vmax, lr, beta1, beta2, eps, step_dev, grad_scale, zero_grad, deferred):
    """GradReducer.deferred + Adam(amsgrad) in one launch (mmvae_adam_fold_flat)"""
    WEIGHT_GEN[0] += 1
    _call("mmvae_adam_fold_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), lr, beta1, beta2, eps,
          H.ptr(step_dev), grad_scale, int(zero_grad), ctypes.byref(deferred["table"]), *_tail_args(deferred["tail"]),
          H.stream())


def adam_fold_range(p, g, m, v, vmax, lo, hi, advance, lr, beta1, beta2, eps, step_dev, grad_scale, zero_grad, table, tail=None):
    """the same over elements [lo, hi) only, with the segments of `table` (H.ReduceSegments or None) that lie inside
    (mmvae_adam_fold_range); advance: this is the launch that closes the step"""
    WEIGHT_GEN[0] += 1
    _call("mmvae_adam_fold_range", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), int(lo), int(hi),
          int(advance), lr, beta1, beta2, eps, H.ptr(step_dev), grad_scale, int(zero_grad),
          ctypes.byref(table) if table is not None else None, *_tail_args(tail), H.stream())


def step_inc(step_dev):
    _call("mmvae_step_inc", H.ptr(step_dev), H.stream())


class Sigmoid(Function):
    @staticmethod
    def forward(ctx, x):
        x = H.f32c(x)
        y = torch.empty_like(x)
        _call("mmvae_sigmoid_fwd", H.ptr(x), H.ptr(y), x.numel(), H.stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        _call("mmvae_sigmoid_bwd", H.ptr(H.f32c(dy)), H.ptr(y), H.ptr(dx), y.numel(), H.stream())
        return dx


def sigmoid(x):
    return Sigmoid.apply(x)


def randn(shape, state):
    """standard-normal tensor from the counter-based device generator (`state`: int32[3] = seed, counter, ticket)"""
    out = torch.empty(shape, device=state.device)
    _call("mmvae_randn", H.ptr(out), out.numel(), H.ptr(state), H.stream())
    return out


def rand_laplace(shape, state):
    """standard-Laplace variates (Laplace.rsample: z = loc + scale * e) from the counter-based device generator"""
    out = torch.empty(shape, device=state.device)
    _call("mmvae_rand_laplace", H.ptr(out), out.numel(), H.ptr(state), H.stream())
    return out


def expand_image_u8(src_u8, dst):
    """dst (fp32, same numel) = src_u8 / 255, bit-identical to torch's true division of the converted bytes"""
    assert src_u8.dtype == torch.uint8 and dst.dtype == torch.float32 and src_u8.numel() == dst.numel()
    assert src_u8.is_contiguous() and dst.is_contiguous()
    _call("mmvae_expand_image_u8", H.ptr(src_u8), H.ptr(dst), dst.numel(), H.stream())
    return dst


def expand_text_tokens(tokens, lengths, onehot, mask_u8=None):
    """tokens (B,T) int32 (-1 = outside the alphabet), lengths (B) int32 -> onehot (B,T,V) fp32, mask (B,T) bytes"""
    assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and onehot.dtype == torch.float32
    B, T, V = onehot.shape
    assert tokens.shape == (B, T) and lengths.shape == (B,) and tokens.is_contiguous() and onehot.is_contiguous()
    _call("mmvae_expand_text_tokens", H.ptr(tokens), H.ptr(lengths), H.ptr(onehot), H.ptr(mask_u8), B, T, V, H.stream())
    return onehot


def fill(t, value):
    _call("mmvae_fill", H.ptr(t), t.numel(), float(value), H.stream())


# ---- held-out log-likelihood estimation (csrc/loglik.hip): forward only, no autograd ------------------------------------
def mix_ksample_logw(comps, laplace, theta, Kc, k0=0, eps=None, rng=None, advance=True, prior_loc=None,
                     prior_laplace=False):
    """Stratified draws from the mixture q = (1/C) sum_c q_c and the latent part of their importance weights.
    comps (C,B,2D) = [loc | scale], laplace: C flags, theta (1,D): the prior's scale is softmax(theta) D.
    Draw k0 + k (k < Kc) comes from component (k0 + k) % C; its noise is eps[k] (eps (Kc,B,D)) or, with `rng` (the
    generator state), element (k0 + k) B D + b D + d of the current draw -- `advance` bumps the state's call counter and
    belongs to the last chunk of a draw.  -> z (Kc,B,D), lw0 (Kc,B) = log p(z) - log q(z)."""
    comps = H.f32c(comps)
    C, B, D2 = comps.shape
    D = D2 // 2
    assert len(laplace) == C and (eps is None) != (rng is None), "either eps or the generator state"
    if eps is not None:
        eps = H.f32c(eps)
        assert tuple(eps.shape) == (Kc, B, D), (tuple(eps.shape), (Kc, B, D))
    if prior_loc is not None:
        prior_loc = H.f32c(prior_loc)
        assert prior_loc.numel() == D
    theta = H.f32c(theta)
    assert theta.numel() == D
    z = torch.empty(Kc, B, D, device=comps.device)
    lw0 = torch.empty(Kc, B, device=comps.device)
    mask = sum(1 << c for c, f in enumerate(laplace) if f)
    _call("mmvae_mix_ksample_logw_fwd", H.ptr(comps), mask, H.ptr(theta), H.ptr(prior_loc), int(bool(prior_laplace)),
          H.ptr(eps), H.ptr(rng), int(bool(advance)), H.ptr(z), H.ptr(lw0), C, int(Kc), int(k0), B, D, H.stream())
    return z, lw0


def lme_state(n_rows, B, device):
    """empty streaming log-sum-exp state (1 + n_rows, 3, B) fp64: running maximum -inf, both sums 0"""
    st = torch.zeros(1 + n_rows, 3, B, dtype=torch.float64, device=device)
    st[:, 0] = float("-inf")
    return st


def lme_update(state, lw0, rows, joint_mask=None):
    """fold one chunk into the state: row 0 takes lw0 + sum of the rows in `joint_mask` (default: all), row 1 + m takes
    rows[m].  lw0 and every row: (Kc,B) fp32."""
    lw0 = H.f32c(lw0)
    Kc, B = lw0.shape
    rows = [H.f32c(r).reshape(-1) for r in rows]
    assert state.dtype == torch.float64 and tuple(state.shape) == (1 + len(rows), 3, B) and state.is_contiguous()
    assert all(r.numel() == Kc * B for r in rows)
    t = H.LmeRows()
    for m, r in enumerate(rows):
        t.ll[m] = r.data_ptr()
    mask = (1 << len(rows)) - 1 if joint_mask is None else int(joint_mask)
    _call("mmvae_lme_update", H.ptr(state), H.ptr(lw0), ctypes.byref(t), len(rows), mask, Kc, B, H.stream())
    return state


def lme_finish(state, K):
    """-> (log-mean-exp over the K folded samples (1 + n_rows, B), effective sample size of row 0 (B,)), fp64"""
    R, _, B = state.shape
    out = torch.empty(R, B, dtype=torch.float64, device=state.device)
    ess = torch.empty(B, dtype=torch.float64, device=state.device)
    _call("mmvae_lme_finish", H.ptr(state), H.ptr(out), H.ptr(ess), R - 1, int(K), B, H.stream())
    return out, ess


# ---- host helpers of the evaluation metrics: labels, and the minibatch `order` of probe_train / digit_train -------------------
def label_matrix(batches, what, who):
    """labels of an iterable of (batch, labels) -> (A, N) int64 on the host; `who` names the caller in the errors"""
    cols = []
    for _, y in batches:
        y = torch.as_tensor(y).detach().cpu()
        if y.is_floating_point() or y.dim() not in (1, 2):
            raise ValueError(f"{who}: {what} labels must be an integer (B,) or (B, A) array")
        cols.append(y.long().reshape(y.shape[0], -1))
    if not cols:
        raise ValueError(f"{who}: the {what} set is empty")
    return torch.cat(cols, 0).t().contiguous()


def epoch_orders(N, epochs, seed, device, shuffle=True):
    """the `order` argument of probe_train / digit_train: (epochs, N) int32 on `device`, one permutation of the N rows per
    epoch drawn from torch.Generator(seed); None -- sequential minibatches -- when not shuffling"""
    if not shuffle:
        return None
    g = torch.Generator().manual_seed(int(seed))
    return torch.stack([torch.randperm(N, generator=g) for _ in range(int(epochs))]).to(device=device, dtype=torch.int32)


def _check_order(who, order, N, batch, step0, n_steps, validate, check_labels):
    """`order` of probe_train / digit_train: (E,N) contiguous int32, E epochs enough for the steps [step0, step0 + n_steps);
    under `validate` the caller's `check_labels()`, then every entry a row in [0, N).  -> E (0: sequential, no `order`)"""
    E = 0
    if order is not None:
        assert order.dim() == 2 and order.dtype == torch.int32 and order.is_contiguous() and order.shape[1] == N
        E = order.shape[0]
        spe = (N + batch - 1) // batch
        if (step0 + n_steps - 1) // spe >= E:
            raise ValueError(f"{who}: steps up to {step0 + n_steps} need more than the {E} epochs of `order`")
    if validate:
        check_labels()
        if order is not None and (int(order.min()) < 0 or int(order.max()) >= N):
            raise ValueError(f"{who}: `order` holds rows outside [0, N)")
    return E


# ---- latent classification (csrc/probe.hip): linear probes trained on chip, forward only, no autograd ---------------------
def _probe_table(probes, Cmax):
    """[(s, a, C)] -> the host (P,3) int table of the C ABI.  The class counts are checked here (ValueError names them);
    the kernels refuse the same shapes with MMVAE_ERR_UNSUPPORTED."""
    probes = [tuple(int(x) for x in pr) for pr in probes]
    if not probes or len(probes) > H.PROBE_MAX_PROBES:
        raise ValueError(f"probe table: {len(probes)} probes (1 .. {H.PROBE_MAX_PROBES} per launch)")
    for s, a, C in probes:
        if not 2 <= C <= min(Cmax, H.PROBE_MAX_CLASSES):
            raise ValueError(f"probe table: {C} classes (2 .. {min(Cmax, H.PROBE_MAX_CLASSES)} are on the MI355X path)")
    flat = [x for pr in probes for x in pr]
    return probes, (ctypes.c_int * len(flat))(*flat)


def _probe_dims(state, z, probes):
    """shape contract shared by probe_train / probe_eval -> (P, S, N, D, Cmax)"""
    assert z.dim() == 3 and z.dtype == torch.float32 and z.is_contiguous(), "z: contiguous fp32 (S,N,D)"
    S, N, D = z.shape
    if D > 256:
        raise ValueError(f"probe: D = {D} latent dimensions (up to 256 are on the MI355X path)")
    assert state.dim() == 4 and state.shape[1] == 3 and state.dtype == torch.float32 and state.is_contiguous()
    P, Cmax = state.shape[0], state.shape[2]
    assert state.shape[3] == D + 1 and P == len(probes), "state: (P, 3, Cmax, D + 1), one row per probe"
    return P, S, N, D, Cmax


def probe_check_labels(labels, probes):
    """ValueError if a probe's label row holds a label outside [0, C) (one host synchronisation)"""
    lo, hi = labels.amin(1).tolist(), labels.amax(1).tolist()
    for s, a, C in probes:
        if not 0 <= int(a) < labels.shape[0]:
            raise ValueError(f"probe table: label row {a} of {labels.shape[0]}")
        if lo[a] < 0 or hi[a] >= C:
            raise ValueError(f"probe labels: row {a} holds labels in [{lo[a]}, {hi[a]}], outside [0, {C})")


def probe_state(P, D, Cmax, device, init=None, seed=0):
    """(P, 3, Cmax, D + 1) fp32: [parameters | exp_avg | exp_avg_sq] per probe, each a (Cmax, D + 1) matrix [W | b].
    nn.Linear's default init -- W and b ~ U(-1/sqrt(D), 1/sqrt(D)) -- drawn on the host from torch.Generator(seed), or
    the (W (C,D), b (C,)) pairs of `init` (rows beyond C stay 0).  The moments start at 0."""
    P, D, Cmax = int(P), int(D), int(Cmax)
    if D < 1 or D > 256:
        raise ValueError(f"probe: D = {D} latent dimensions (1 .. 256 are on the MI355X path)")
    if not 2 <= Cmax <= H.PROBE_MAX_CLASSES:
        raise ValueError(f"probe: {Cmax} classes (2 .. {H.PROBE_MAX_CLASSES} are on the MI355X path)")
    par = torch.zeros(P, Cmax, D + 1)
    if init is None:
        bound = 1.0 / D ** 0.5
        g = torch.Generator().manual_seed(int(seed))
        par.copy_((torch.rand(P, Cmax, D + 1, generator=g) * 2.0 - 1.0) * bound)
    else:
        assert len(init) == P, "init: one (W, b) pair per probe"
        for p, (W, b) in enumerate(init):
            C = W.shape[0]
            assert W.shape == (C, D) and b.shape == (C,) and C <= Cmax, (tuple(W.shape), tuple(b.shape), Cmax, D)
            par[p, :C, :D] = W.detach().float().cpu()
            par[p, :C, D] = b.detach().float().cpu()
    state = torch.zeros(P, 3, Cmax, D + 1)
    state[:, 0] = par
    return state.to(device)


def probe_weights(state, p, C):
    """-> (W (C,D), b (C,)) of probe p (copies)"""
    par = state[p, 0, :C]
    return par[:, :-1].clone(), par[:, -1].clone()


def probe_train(state, z, labels, probes, batch, step0, n_steps, lr=1e-3, order=None, validate=True):
    """Adam steps [step0, step0 + n_steps) of every probe in ONE launch (one workgroup per probe), in place on `state`.
    z (S,N,D) fp32, labels (A,N) int32, probes [(s, a, C)]; step t covers positions [i batch, (i + 1) batch) of epoch
    t // ceil(N / batch); `order` (E,N) int32 maps position -> row per epoch (None: sequential).
    -> loss (P, n_steps): the mean cross-entropy of every step.  `validate`: check labels / order on the host first."""
    P, S, N, D, Cmax = _probe_dims(state, z, probes)
    probes, table = _probe_table(probes, Cmax)
    assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[1] == N
    if int(batch) < 1 or int(n_steps) < 1 or int(step0) < 0:
        raise ValueError(f"probe_train: batch = {batch}, step0 = {step0}, n_steps = {n_steps}")
    E = _check_order("probe_train", order, N, int(batch), int(step0), int(n_steps), validate,
                     lambda: probe_check_labels(labels, probes))
    for s, a, C in probes:
        if not (0 <= s < S and 0 <= a < labels.shape[0]):
            raise ValueError(f"probe table: probe ({s}, {a}, {C}) outside {S} latent matrices / {labels.shape[0]} label rows")
    loss = torch.empty(P, int(n_steps), device=z.device)
    _call("mmvae_probe_train", H.ptr(state), H.ptr(z), H.ptr(labels), H.ptr(order), E, table, H.ptr(loss), P, S,
          labels.shape[0], N, D, Cmax, int(batch), int(step0), int(n_steps), float(lr), H.stream())
    return loss


def probe_eval(state, z, labels, probes):
    """-> (pred (P,N) int32: argmax of the logits, the first maximum; nll (P,N) fp32: the row's cross-entropy against its
    probe's label row, 0 when `labels` is None)"""
    P, S, N, D, Cmax = _probe_dims(state, z, probes)
    probes, table = _probe_table(probes, Cmax)
    A = 0
    if labels is not None:
        assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[1] == N
        A = labels.shape[0]
    for s, a, C in probes:
        if not (0 <= s < S and (labels is None or 0 <= a < A)):
            raise ValueError(f"probe table: probe ({s}, {a}, {C}) outside {S} latent matrices / {A} label rows")
    pred = torch.empty(P, N, dtype=torch.int32, device=z.device)
    nll = torch.empty(P, N, device=z.device)
    _call("mmvae_probe_eval", H.ptr(state), H.ptr(z), H.ptr(labels), table, H.ptr(pred), H.ptr(nll), P, S, A, N, D, Cmax,
          H.stream())
    return pred, nll


# ---- generation coherence (csrc/coherence.hip): scoring kernels, forward only, no autograd -------------------------------
def text_decode_score(logits, target_ids=None, lengths=None):
    """logits (N,T,V) fp32 -> pred (N,T) int32: the first maximum over V of every step (an all-zero row gives 0).
    With target_ids (N,T) int32 and lengths (N,) int32 also letters (N,) int32: the steps t < min(lengths[n], T) at which
    pred equals the target (None without targets)."""
    assert logits.dim() == 3 and logits.dtype == torch.float32, "logits: fp32 (N,T,V)"
    logits = logits.contiguous()
    N, T, V = logits.shape
    if not (1 <= T <= H.COH_MAX_STEPS and 2 <= V <= H.COH_MAX_VOCAB):
        raise ValueError(f"text_decode_score: T = {T}, V = {V} (1 .. {H.COH_MAX_STEPS} steps, 2 .. {H.COH_MAX_VOCAB} "
                         f"symbols are on the MI355X path)")
    if (target_ids is None) != (lengths is None):
        raise ValueError("text_decode_score: target_ids and lengths come together")
    pred = torch.empty(N, T, dtype=torch.int32, device=logits.device)
    letters = None
    if N == 0:
        return pred, (None if target_ids is None else torch.empty(0, dtype=torch.int32, device=logits.device))
    if target_ids is not None:
        assert target_ids.shape == (N, T) and target_ids.dtype == torch.int32 and target_ids.is_contiguous()
        assert lengths.shape == (N,) and lengths.dtype == torch.int32 and lengths.is_contiguous()
        letters = torch.empty(N, dtype=torch.int32, device=logits.device)
    _call("mmvae_text_decode_score", H.ptr(logits), H.ptr(target_ids), H.ptr(lengths), H.ptr(pred), H.ptr(letters), N, T,
          V, H.stream())
    return pred, letters


def cls_head(feats, W1, b1, W2, b2, n_classes, labels=None, want_logits=False):
    """The heads of A attribute classifiers in one launch.  feats (A,N,512): the trunks' last conv output before its
    ReLU; W1 (A,256,512), b1 (A,256), W2 (A,Cmax,256), b2 (A,Cmax); n_classes: A ints; labels (A,N) int32 or None
    (-1: never correct).  -> {"pred" (A,N) int32, "logits" (A,N,Cmax) or None, "correct" (A,N) uint8 and "n_correct"
    (N,) int32 (None without labels)}."""
    assert feats.dim() == 3 and feats.dtype == torch.float32 and feats.is_contiguous(), "feats: contiguous fp32 (A,N,512)"
    A, N, F_ = feats.shape
    n_classes = [int(c) for c in n_classes]
    Cmax = W2.shape[1]
    if not 1 <= A <= H.COH_MAX_CLASSIFIERS or len(n_classes) != A:
        raise ValueError(f"cls_head: {A} classifiers, {len(n_classes)} class counts (1 .. {H.COH_MAX_CLASSIFIERS} per "
                         f"launch)")
    if not 2 <= Cmax <= H.COH_MAX_CLASSES or any(not 2 <= c <= Cmax for c in n_classes):
        raise ValueError(f"cls_head: class counts {n_classes} under Cmax = {Cmax} (2 .. {H.COH_MAX_CLASSES} are on the "
                         f"MI355X path)")
    assert F_ == H.COH_FEATS and W1.shape == (A, H.COH_HIDDEN, H.COH_FEATS) and b1.shape == (A, H.COH_HIDDEN)
    assert W2.shape == (A, Cmax, H.COH_HIDDEN) and b2.shape == (A, Cmax)
    for t in (W1, b1, W2, b2):
        assert t.dtype == torch.float32 and t.is_contiguous(), "cls_head: contiguous fp32 parameters"
    dev = feats.device
    pred = torch.empty(A, N, dtype=torch.int32, device=dev)
    logits = torch.empty(A, N, Cmax, device=dev) if want_logits else None
    correct = n_correct = None
    if labels is not None:
        assert labels.shape == (A, N) and labels.dtype == torch.int32 and labels.is_contiguous(), "labels: int32 (A,N)"
        correct = torch.empty(A, N, dtype=torch.uint8, device=dev)
        n_correct = torch.empty(N, dtype=torch.int32, device=dev)
    if N > 0:
        _call("mmvae_cls_head", H.ptr(feats), H.ptr(W1), H.ptr(b1), H.ptr(W2), H.ptr(b2), (ctypes.c_int * A)(*n_classes),
              H.ptr(labels), H.ptr(pred), H.ptr(logits), H.ptr(correct), H.ptr(n_correct), A, N, Cmax, H.stream())
    return {"pred": pred, "logits": logits, "correct": correct, "n_correct": n_correct}


# ---- MNIST-SVHN digit classifiers (csrc/digits.hip): evaluated and trained on chip, no autograd ---------------------------
DIGIT_KINDS = {"mnist": H.DIGIT_MNIST, "svhn": H.DIGIT_SVHN}
DIGIT_INPUT = {"mnist": (1, 28, 28), "svhn": (3, 32, 32)}
DIGIT_N_PARAMS = {"mnist": 21840, "svhn": 31340}


def digit_param_shapes(kind):
    """[(state-dict key, shape)] of a digit classifier in the packed order of the C ABI (the reference's module names)"""
    C, flat = DIGIT_INPUT[kind][0], (320 if kind == "mnist" else 500)
    return [("conv1.weight", (10, C, 5, 5)), ("conv1.bias", (10,)), ("conv2.weight", (20, 10, 5, 5)), ("conv2.bias", (20,)),
            ("fc1.weight", (50, flat)), ("fc1.bias", (50,)), ("fc2.weight", (10, 50)), ("fc2.bias", (10,))]


def _digit_kinds(kinds):
    kinds = [kinds] if isinstance(kinds, str) else list(kinds)
    if not 1 <= len(kinds) <= H.DIGIT_MAX_NETS or any(k not in DIGIT_KINDS for k in kinds):
        raise ValueError(f"digit classifiers: kinds = {kinds} (1 .. {H.DIGIT_MAX_NETS} of 'mnist' / 'svhn')")
    return kinds


def digit_default_init(kind, generator):
    """nn.Conv2d's / nn.Linear's default init -- weight and bias ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)) -- drawn on the
    host from `generator`, in the packed order -> {key: tensor}"""
    out = {}
    shapes = digit_param_shapes(kind)
    for (kw, sw), (kb, sb) in zip(shapes[0::2], shapes[1::2]):
        fan_in = 1
        for s in sw[1:]:
            fan_in *= s
        bound = 1.0 / fan_in ** 0.5
        out[kw] = (torch.rand(*sw, generator=generator) * 2.0 - 1.0) * bound
        out[kb] = (torch.rand(*sb, generator=generator) * 2.0 - 1.0) * bound
    return out


def digit_pack(kind, params):
    """{key: tensor} -> the packed (n_params,) fp32 host vector"""
    parts = []
    for k, s in digit_param_shapes(kind):
        t = params[k].detach().float().cpu()
        assert tuple(t.shape) == s, (k, tuple(t.shape), s)
        parts.append(t.reshape(-1))
    return torch.cat(parts)


def digit_unpack(kind, vec):
    """a packed (>= n_params,) vector -> {key: tensor} (copies, on vec's device)"""
    out, o = {}, 0
    for k, s in digit_param_shapes(kind):
        n = 1
        for d in s:
            n *= d
        out[k] = vec[o:o + n].reshape(s).clone()
        o += n
    return out


def digit_state(kinds, device, init=None, seed=0):
    """(nets, 3, n_params_max) fp32: [parameters | exp_avg | exp_avg_sq] per network in the packed order conv1.w, conv1.b,
    conv2.w, conv2.b, fc1.w, fc1.b, fc2.w, fc2.b.  The init is nn.Conv2d's / nn.Linear's default, drawn on the host from
    torch.Generator(seed) network after network, or `init`: one {state-dict key: tensor} per network.  Moments start at 0."""
    kinds = _digit_kinds(kinds)
    stride = max(DIGIT_N_PARAMS[k] for k in kinds)
    state = torch.zeros(len(kinds), 3, stride)
    g = torch.Generator().manual_seed(int(seed))
    if init is not None:
        assert len(init) == len(kinds), "init: one parameter dict per network"
    for i, k in enumerate(kinds):
        par = digit_default_init(k, g) if init is None else init[i]
        state[i, 0, :DIGIT_N_PARAMS[k]] = digit_pack(k, par)
    return state.to(device)


def _digit_args(state, kinds, images, labels=None):
    """shape contract of the digit entry points -> (kinds, host kind table, image pointer table, label pointer table, N)"""
    kinds = _digit_kinds(kinds)
    nets = len(kinds)
    assert state.dim() == 3 and state.shape[:2] == (nets, 3) and state.dtype == torch.float32 and state.is_contiguous(), \
        "state: contiguous fp32 (nets, 3, n_params_max)"
    assert state.shape[2] >= max(DIGIT_N_PARAMS[k] for k in kinds), "state: narrower than the largest network"
    assert len(images) == nets, "images: one (N,C,H,W) tensor per network"
    N = images[0].shape[0]
    for k, x in zip(kinds, images):
        assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (N,) + DIGIT_INPUT[k], \
            f"{k} images: contiguous fp32 (N,{','.join(map(str, DIGIT_INPUT[k]))}), got {tuple(x.shape)}"
    lab = None
    if labels is not None:
        assert len(labels) == nets, "labels: one (N,) int32 tensor per network"
        for y in labels:
            assert y.dtype == torch.int32 and y.is_contiguous() and tuple(y.shape) == (N,), "labels: contiguous int32 (N,)"
        lab = (H.c_p * nets)(*[H.ptr(y) for y in labels])
    return kinds, (ctypes.c_int * nets)(*[DIGIT_KINDS[k] for k in kinds]), (H.c_p * nets)(*[H.ptr(x) for x in images]), lab, N


def digit_check_labels(labels):
    """ValueError if a label lies outside [0, 10) (one host synchronisation per tensor)"""
    for y in labels:
        lo, hi = int(y.min()), int(y.max())
        if lo < 0 or hi >= 10:
            raise ValueError(f"digit classifiers: labels in [{lo}, {hi}], outside [0, 10)")


def _digit_p(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"digit classifiers: dropout p = {p} (0 <= p < 1)")
    return p


def digit_eval(state, kinds, images):
    """-> (logp (nets,N,10) fp32 log-probabilities, pred (nets,N) int32: their first maximum); dropout off"""
    kinds, ktab, xtab, _, N = _digit_args(state, kinds, images)
    dev = state.device
    logp = torch.empty(len(kinds), N, 10, device=dev)
    pred = torch.empty(len(kinds), N, dtype=torch.int32, device=dev)
    if N > 0:
        _call("mmvae_digit_eval", H.ptr(state), ktab, xtab, H.ptr(logp), H.ptr(pred), len(kinds), state.shape[2], N,
              H.stream())
    return logp, pred


def digit_grad(state, kinds, images, labels, seed=0, step=0, p=0.0, validate=True):
    """The first half of a training step on one minibatch (all N rows of `images`): -> (grad (nets, n_params_max): the
    gradient of the mean loss with the dropout masks of (seed, step), rowloss (nets,N) = -logp[label])"""
    kinds, ktab, xtab, ltab, N = _digit_args(state, kinds, images, labels)
    if not 1 <= N <= 65535:
        raise ValueError(f"digit_grad: a minibatch of {N} rows (1 .. 65535)")
    if validate:
        digit_check_labels(labels)
    nets, stride, dev = len(kinds), state.shape[2], state.device
    ws = H.workspace(H.lib().mmvae_digit_ws_floats(nets, N, stride), dev)
    grad = torch.zeros(nets, stride, device=dev)
    rowloss = torch.empty(nets, N, device=dev)
    _call("mmvae_digit_grad", H.ptr(state), ktab, xtab, ltab, H.ptr(ws), H.ptr(grad), H.ptr(rowloss), nets, stride, N,
          int(seed) & 0xFFFFFFFF, int(step), _digit_p(p), H.stream())
    return grad, rowloss


def digit_train(state, kinds, images, labels, batch, step0, n_steps, lr=1e-3, seed=0, p=0.5, order=None, validate=True):
    """Adam steps [step0, step0 + n_steps) of every network, in place on `state`: forward with dropout, backward, Adam;
    two launches per step.  images: per network (N,C,H,W) fp32 on the device, labels: per network (N,) int32; the
    minibatch schedule and `order` (E,N) int32 are ops.probe_train's.  -> loss (nets, n_steps)."""
    kinds, ktab, xtab, ltab, N = _digit_args(state, kinds, images, labels)
    batch, step0, n_steps = int(batch), int(step0), int(n_steps)
    if not 1 <= batch <= 65535 or n_steps < 1 or step0 < 0 or N < 1:
        raise ValueError(f"digit_train: batch = {batch}, step0 = {step0}, n_steps = {n_steps}, N = {N}")
    E = _check_order("digit_train", order, N, batch, step0, n_steps, validate, lambda: digit_check_labels(labels))
    nets, stride, dev = len(kinds), state.shape[2], state.device
    ws = H.workspace(H.lib().mmvae_digit_ws_floats(nets, batch, stride), dev)
    loss = torch.empty(nets, n_steps, device=dev)
    _call("mmvae_digit_train", H.ptr(state), ktab, xtab, ltab, H.ptr(order), E, H.ptr(ws), H.ptr(loss), nets, stride, N,
          batch, step0, n_steps, float(lr), int(seed) & 0xFFFFFFFF, _digit_p(p), H.stream())
    return loss


def digit_masks(kind, batch, step0, n_steps, seed=0, p=0.5, device="cuda"):
    """The masks digit_train / digit_grad use for the steps [step0, step0 + n_steps) of a network kind, as 0 or 1/(1-p)
    floats -> (Dropout2d mask (n_steps, batch, 20), dropout mask (n_steps, batch, 50))"""
    (kind,) = _digit_kinds(kind)
    batch, n_steps = int(batch), int(n_steps)
    if not 1 <= batch <= 65535 or n_steps < 1 or int(step0) < 0:
        raise ValueError(f"digit_masks: batch = {batch}, step0 = {step0}, n_steps = {n_steps}")
    m2d = torch.empty(n_steps, batch, 20, device=device)
    m1 = torch.empty(n_steps, batch, 50, device=device)
    _call("mmvae_digit_masks", H.ptr(m2d), H.ptr(m1), DIGIT_KINDS[kind], int(seed) & 0xFFFFFFFF, int(step0), n_steps,
          batch, _digit_p(p), H.stream())
    return m2d, m1


# ---- latent analysis (csrc/tsne.hip): exact t-SNE, forward only, no autograd ------------------------------------------------
TSNE_SWITCH_IT = 250      # iterations with early exaggeration 12 and momentum 0.5 (scikit-learn's _EXPLORATION_MAX_ITER)
TSNE_CHECK_EVERY = 50     # iterations per enqueued call and between two looks at the log (its _N_ITER_CHECK)


def _tsne_points(who, X):
    assert X.dim() == 2 and X.dtype == torch.float32, f"{who}: fp32 (N, D)"
    N, D = X.shape
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS or not 1 <= D <= H.TSNE_MAX_DIM:
        raise ValueError(f"{who}: N = {N} points of D = {D} dimensions ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} points "
                         f"of 1 .. {H.TSNE_MAX_DIM} dimensions are on the MI355X path)")
    return N, D


def tsne_sqdist(X):
    """X (N,D) fp32 -> D2 (N,N) fp32: the squared Euclidean distances, every one summed directly in double and rounded
    (no Gram trick: near-duplicates do not cancel); zero diagonal, symmetric bit for bit."""
    N, D = _tsne_points("tsne_sqdist", X)
    X = X.contiguous()
    D2 = torch.empty(N, N, device=X.device)
    _call("mmvae_tsne_sqdist", H.ptr(X), H.ptr(D2), N, D, H.stream())
    return D2


def tsne_default_init(N, seed=123):
    """scikit-learn's init="random": 1e-4 * RandomState(seed).standard_normal((N, 2)) as float32 (a host tensor)"""
    return torch.from_numpy((1e-4 * np.random.RandomState(int(seed)).standard_normal((int(N), 2))).astype(np.float32))


def tsne_check_perplexity(perplexity, N):
    if not float(perplexity) > 0.0:
        raise ValueError(f"perplexity must be positive, got {perplexity}")
    if float(perplexity) >= N:
        raise ValueError("perplexity must be less than n_samples")


def tsne_joint_probabilities(X, perplexity, sqdist=None, details=False):
    """-> (P (N,N) fp32, beta (N,) float64): scikit-learn's _joint_probabilities of the squared distances of X (or of
    `sqdist` (N,N) fp32 as given) -- per row the binary search for the precision beta that gives the conditional
    distribution the entropy log(perplexity), in double; P = max((C + C^T) / sum, eps) off the diagonal, 0 on it,
    symmetric bit for bit.  P is a view of rows padded to a multiple of 4 columns, the layout the iteration kernels read.
    `details`: also {"s", "rowsum", "steps"} of the search, (N,) float64 each."""
    D2 = tsne_sqdist(X) if sqdist is None else sqdist.contiguous()
    assert D2.dim() == 2 and D2.shape[0] == D2.shape[1] and D2.dtype == torch.float32, "sqdist: fp32 (N,N)"
    N = D2.shape[0]
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS:
        raise ValueError(f"tsne_joint_probabilities: N = {N} points ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} are on the "
                         f"MI355X path)")
    tsne_check_perplexity(perplexity, N)
    ld = H.lib().mmvae_tsne_ld(N)
    store = torch.empty(N, ld, device=D2.device)
    info = torch.empty(N, 4, dtype=torch.float64, device=D2.device)
    total = torch.empty(1, dtype=torch.float64, device=D2.device)
    _call("mmvae_tsne_joint_p", H.ptr(D2), float(perplexity), H.ptr(store), ld, H.ptr(info), H.ptr(total), N, H.stream())
    P = store[:, :N]
    if details:
        return P, info[:, 0].clone(), {"s": info[:, 1].clone(), "rowsum": info[:, 2].clone(), "steps": info[:, 3].clone()}
    return P, info[:, 0].clone()


def _tsne_padded(P):
    """P (N,N) fp32 as the kernels read it: unit column stride, a row stride of N rounded up to 4 (16-byte rows) -- the
    view tsne_joint_probabilities returns as it is, anything else copied into that layout"""
    assert P.dim() == 2 and P.shape[0] == P.shape[1] and P.dtype == torch.float32, "P: fp32 (N,N)"
    N = P.shape[0]
    ld = (N + 3) & ~3
    if P.stride(1) == 1 and P.stride(0) == ld and P.data_ptr() % 16 == 0:
        return P, ld
    store = torch.zeros(N, ld, device=P.device)
    store[:, :N] = P
    return store[:, :N], ld


def tsne_state(Y0):
    """Y0 (N,2) -> the iteration's state (3,N,2) fp32 on the device Y0 is on: Y | upd = 0 | gains = 1"""
    assert Y0.dim() == 2 and Y0.shape[1] == 2, "Y0: (N,2)"
    Y0 = Y0.detach().float()
    return torch.stack([Y0, torch.zeros_like(Y0), torch.ones_like(Y0)]).contiguous()


def _tsne_args(who, state, P):
    assert state.dim() == 3 and state.shape[0] == 3 and state.shape[2] == 2 and state.dtype == torch.float32 \
        and state.is_contiguous(), "state: contiguous fp32 (3,N,2) from tsne_state"
    N = state.shape[1]
    if not H.TSNE_MIN_POINTS <= N <= H.TSNE_MAX_POINTS:
        raise ValueError(f"{who}: N = {N} points ({H.TSNE_MIN_POINTS} .. {H.TSNE_MAX_POINTS} are on the MI355X path)")
    assert P.shape[0] == N, f"{who}: P is {tuple(P.shape)}, the state holds {N} points"
    P, ld = _tsne_padded(P)
    ws = torch.empty(H.lib().mmvae_tsne_ws_doubles(N), dtype=torch.float64, device=state.device)
    return N, P, ld, ws


def tsne_forces(state, P, it, switch_it=TSNE_SWITCH_IT):
    """The first half of iteration `it` (exaggeration 12 for it < switch_it, then 1), the state untouched
    -> (g (N,2) fp32: the gradient of the objective, KL, Z: 0-d float64 tensors on the device)."""
    N, P, ld, ws = _tsne_args("tsne_forces", state, P)
    g = torch.empty(N, 2, device=state.device)
    kz = torch.empty(2, dtype=torch.float64, device=state.device)
    _call("mmvae_tsne_forces", H.ptr(state), H.ptr(P), ld, H.ptr(ws), H.ptr(g), H.ptr(kz), N, int(it), int(switch_it),
          H.stream())
    return g, kz[0], kz[1]


def tsne_default_lr(N):
    """scikit-learn's learning_rate="auto": max(N / early_exaggeration / 4, 50)"""
    return max(N / 12.0 / 4.0, 50.0)


def tsne_run(state, P, it0, n_iter, lr, switch_it=TSNE_SWITCH_IT, kl_every=1):
    """The iterations [it0, it0 + n_iter) in place on `state`, enqueued in one call (two launches per iteration, no host
    synchronisation) -> log (n_iter,2) float64 on the device: (KL with the iteration's exaggeration, |g|_2) at the
    embedding each iteration started from.  `kl_every`: KL is computed in the iterations with (it + 1) % kl_every == 0,
    NaN elsewhere (scikit-learn computes it every 50th; its double logarithms are most of a pair's arithmetic).
    Bit-identical from run to run and however the iterations are split over calls."""
    N, P, ld, ws = _tsne_args("tsne_run", state, P)
    if int(n_iter) < 1 or int(it0) < 0 or not float(lr) > 0.0 or int(kl_every) < 1:
        raise ValueError(f"tsne_run: it0 = {it0}, n_iter = {n_iter}, lr = {lr}, kl_every = {kl_every}")
    log = torch.empty(int(n_iter), 2, dtype=torch.float64, device=state.device)
    _call("mmvae_tsne_run", H.ptr(state), H.ptr(P), ld, H.ptr(ws), H.ptr(log), N, int(it0), int(n_iter), int(switch_it),
          float(lr), int(kl_every), H.stream())
    return log


def tsne_embed(X, perplexity=30.0, max_iter=1000, seed=123, init=None, lr="auto", n_iter_without_progress=300,
               min_grad_norm=1e-7, kl_every=TSNE_CHECK_EVERY):
    """Exact t-SNE of X (N,D) fp32 into two dimensions: sklearn.manifold.TSNE(n_components=2, method="exact",
    init="random", random_state=seed, learning_rate="auto") -- 250 iterations with early exaggeration 12 and momentum 0.5,
    then momentum 0.8 up to `max_iter`, with scikit-learn's stopping rule: every 50th iteration a stage ends when the
    objective has had no new best for more than `n_iter_without_progress` iterations (250 in the first stage) or when
    |g|_2 <= min_grad_norm.  (scikit-learn takes the norm of the gradient scaled by the gains; here it is the gradient's.)
    `init`: (N,2) instead of the seeded draw.  The host enqueues 50 iterations per call and reads the log back once per
    call: at most max_iter / 50 synchronisations.
    -> {"embedding": (N,2) fp32, "kl_divergence": float, the objective at the returned embedding without exaggeration,
        "n_iter": iterations run, "log": (n_iter,2) float64 (KL, |g|) per iteration (KL every `kl_every`-th, NaN between),
        "beta": (N,) float64 precisions of the perplexity search}."""
    N, _ = _tsne_points("tsne_embed", X)
    tsne_check_perplexity(perplexity, N)
    max_iter = int(max_iter)
    if max_iter < TSNE_SWITCH_IT:
        raise ValueError(f"tsne_embed: max_iter = {max_iter} (at least the {TSNE_SWITCH_IT} iterations of the first stage)")
    if TSNE_CHECK_EVERY % int(kl_every) != 0:
        raise ValueError(f"tsne_embed: kl_every = {kl_every} must divide the check cadence {TSNE_CHECK_EVERY}")
    if not bool(torch.isfinite(X).all()):
        raise ValueError("tsne_embed: X holds values that are not finite")
    lr = tsne_default_lr(N) if isinstance(lr, str) else float(lr)
    P, beta = tsne_joint_probabilities(X, perplexity)
    Y0 = tsne_default_init(N, seed) if init is None else torch.as_tensor(init)
    if tuple(Y0.shape) != (N, 2):
        raise ValueError(f"tsne_embed: init is {tuple(Y0.shape)}, not ({N}, 2)")
    state = tsne_state(Y0.to(X.device))
    logs, it, switch_it = [], 0, TSNE_SWITCH_IT
    for stage_end, patience in ((TSNE_SWITCH_IT, TSNE_SWITCH_IT), (max_iter, int(n_iter_without_progress))):
        best, best_it, stop = float("inf"), it, False
        while it < stage_end and not stop:
            n = min(TSNE_CHECK_EVERY - it % TSNE_CHECK_EVERY, stage_end - it)
            log = tsne_run(state, P, it, n, lr, switch_it=switch_it, kl_every=kl_every)
            logs.append(log)
            it += n
            if it % TSNE_CHECK_EVERY == 0:
                kl, gnorm = log[-1].tolist()      # (the synchronisation of this call)
                if kl < best:
                    best, best_it = kl, it - 1
                elif it - 1 - best_it > patience:
                    stop = True
                if gnorm <= float(min_grad_norm):
                    stop = True
        switch_it = min(switch_it, it)
    _, kl, _ = tsne_forces(state, P, max(it, switch_it), switch_it=switch_it)
    return {"embedding": state[0].clone(), "kl_divergence": float(kl), "n_iter": it, "log": torch.cat(logs),
            "beta": beta}


# ---- checks shared by the feature-set metrics (Frechet, manifold, KID) and the chunked kernels --------------------------------
def _feature_rows(who, what, X, least=1, most=None, why="", finite=True):
    """contiguous fp32 (rows, F) or ValueError: shape, dtype, the limit on F, `least` .. `most` rows (`why`: the caller's
    clause on that limit), finite values (`finite` False: the caller checks them after its own comparisons)"""
    if not torch.is_tensor(X) or X.dim() != 2 or not X.is_floating_point():
        said = f"{tuple(X.shape)}, {X.dtype}" if torch.is_tensor(X) else type(X).__name__
        raise ValueError(f"{who}: {what} is {said}; floating (rows, F) features")
    rows, F = X.shape
    if not 1 <= F <= H.FRECHET_MAX_F:
        raise ValueError(f"{who}: {what} has F = {F} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)")
    if rows < least or (most is not None and rows > most):
        raise ValueError(f"{who}: {what} has {rows} rows ({why})")
    X = H.f32c(X.detach())
    if finite:
        _finite(who, what, X)
    return X


def _finite(who, what, X):
    if not bool(torch.isfinite(X).all()):
        raise ValueError(f"{who}: {what} holds values that are not finite")


def _chunks(who, chunks, what="column chunks"):
    chunks = int(chunks)
    if chunks < 0:
        raise ValueError(f"{who}: chunks = {chunks} (0: the default plan, or a positive number of {what})")
    return chunks


# ---- Frechet distance of feature sets (csrc/frechet.hip): float64, forward only, no autograd --------------------------------
def _frechet_f(who, F):
    F = int(F)
    if not 1 <= F <= H.FRECHET_MAX_F:
        raise ValueError(f"{who}: F = {F} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)")
    return F


def _frechet_state_f(who, state):
    """F of a moment state, or ValueError: the contiguous float64 vector (1 + F + F F,) that frechet_state returns"""
    ok = torch.is_tensor(state) and state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous()
    F = (math.isqrt(max(4 * state.numel() - 3, 0)) - 1) // 2 if ok else 0
    if not ok or 1 + F + F * F != state.numel() or not 1 <= F <= H.FRECHET_MAX_F:
        what = f"{tuple(state.shape)}, {state.dtype}" if torch.is_tensor(state) else type(state).__name__
        raise ValueError(f"{who}: the state is {what}; frechet_state gives a contiguous float64 vector (1 + F + F F,), "
                         f"1 <= F <= {H.FRECHET_MAX_F} on the MI355X path")
    return F


def frechet_state(F, device):
    """empty streaming moment state, float64 (1 + F + F F,): n | mean (F) | M2 (F,F), all 0"""
    F = _frechet_f("frechet_state", F)
    return torch.zeros(1 + F + F * F, dtype=torch.float64, device=device)


def frechet_update(state, feats):
    """fold the rows of feats (n_b, F) into the state: batch mean and centred scatter in double (one tiled SYRK on the
    fp64 MFMA), merged by Chan's rule.  Memory does not grow with the number of rows folded."""
    F = _frechet_state_f("frechet_update", state)
    feats = _feature_rows("frechet_update", "feats", feats, least=0, finite=False)
    if feats.shape[1] != F:
        raise ValueError(f"frechet_update: feats has F = {feats.shape[1]} features; the state holds floating (rows, {F})")
    if feats.shape[0] == 0:
        return state
    _finite("frechet_update", "feats", feats)
    ws = torch.empty(F, dtype=torch.float64, device=state.device)
    _call("mmvae_frechet_update", H.ptr(state), H.ptr(feats), H.ptr(ws), feats.shape[0], F, H.stream())
    return state


def frechet_moments(state):
    """-> (n, mu (F,) float64, sigma (F,F) float64 = M2 / (n - 1): np.cov's normalisation, n >= 2)"""
    F = _frechet_state_f("frechet_moments", state)
    n = int(state[0])
    if n < 2:
        raise ValueError(f"frechet_moments: n = {n} rows folded (a covariance needs n >= 2)")
    mu = torch.empty(F, dtype=torch.float64, device=state.device)
    sigma = torch.empty(F, F, dtype=torch.float64, device=state.device)
    _call("mmvae_frechet_finish", H.ptr(state), H.ptr(mu), H.ptr(sigma), n, F, H.stream())
    return n, mu, sigma


def _f64_square(who, what, M):
    if M.dim() != 2 or M.shape[0] != M.shape[1] or M.dtype != torch.float64:
        raise ValueError(f"{who}: {what} of shape {tuple(M.shape)}, {M.dtype}; float64 (F,F), 1 <= F <= {H.FRECHET_MAX_F} on "
                         f"the MI355X path")
    _frechet_f(who, M.shape[0])
    return M.contiguous()


def f64_gemm(A, B, trans_b=False):
    """C = A B (or A B^T) of row-major float64 (F,F) matrices on the fp64 MFMA tile routine"""
    A, B = _f64_square("f64_gemm", "A", A), _f64_square("f64_gemm", "B", B)
    if A.shape != B.shape:
        raise ValueError(f"f64_gemm: A {tuple(A.shape)} and B {tuple(B.shape)} differ")
    C = torch.empty_like(A)
    _call("mmvae_f64_gemm", H.ptr(A), H.ptr(B), H.ptr(C), A.shape[0], int(bool(trans_b)), H.stream())
    return C


def sym_eig(S, vectors=True, max_sweeps=H.EIG_MAX_SWEEPS):
    """One-sided Jacobi of the symmetric float64 S (F,F) in round-robin order, one launch per step (include/mmvae_hip.h:
    mmvae_sym_eig) -> {"values": (F,) = |A_j|, the eigenvalues of a positive semi-definite S, unsorted, "vectors": (F,F)
    with column j the eigenvector of values[j] (None for vectors=False: the same values bit for bit), "sweeps": int,
    "rotations": [counted rotations per sweep]}.  The host reads one integer per sweep.  RuntimeError when the sweeps reach
    `max_sweeps` (at most 30) without converging."""
    S = _f64_square("sym_eig", "S", S)
    F, max_sweeps = S.shape[0], int(max_sweeps)
    if not 1 <= max_sweeps <= H.EIG_MAX_SWEEPS:
        raise ValueError(f"sym_eig: max_sweeps = {max_sweeps} (1 .. {H.EIG_MAX_SWEEPS})")
    if not bool(torch.isfinite(S).all()):
        raise ValueError("sym_eig: S holds values that are not finite")
    dev = S.device
    ws = torch.empty(H.lib().mmvae_sym_eig_ws_doubles(F), dtype=torch.float64, device=dev)
    Vc = torch.empty(F, F, dtype=torch.float64, device=dev) if vectors else None
    values = torch.empty(F, dtype=torch.float64, device=dev)
    sweeps, rot = ctypes.c_int(0), (ctypes.c_int * max_sweeps)()
    _call("mmvae_sym_eig", H.ptr(S), H.ptr(ws), H.ptr(Vc), H.ptr(values), ctypes.byref(sweeps), rot, F, max_sweeps,
          H.stream())
    return {"values": values, "vectors": None if Vc is None else Vc.t(), "sweeps": sweeps.value,
            "rotations": list(rot[:sweeps.value])}


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 of float64 moments on the device, the square root through two
    symmetric eigendecompositions: (lambda, V) of S1, R = diag(sqrt(lambda)) V^T, G = R S2 R^T, tr (S1 S2)^1/2 = sum_j
    sqrt(sigma_j(G)).  -> {"distance": float64 0-d tensor, "tr_covmean": float64 0-d tensor, "sweeps": (s1, s2)}."""
    sigma1, sigma2 = _f64_square("frechet_distance", "sigma1", sigma1), _f64_square("frechet_distance", "sigma2", sigma2)
    F = sigma1.shape[0]
    for what, t, shape in (("mu1", mu1, (F,)), ("mu2", mu2, (F,)), ("sigma2", sigma2, (F, F))):
        if tuple(t.shape) != shape or t.dtype != torch.float64:
            raise ValueError(f"frechet_distance: {what} of shape {tuple(t.shape)}, {t.dtype}; float64 {shape} beside sigma1 "
                             f"(1 .. {H.FRECHET_MAX_F} features are on the MI355X path)")
    mu1, mu2 = mu1.contiguous(), mu2.contiguous()
    if not all(bool(torch.isfinite(t).all()) for t in (mu1, mu2, sigma1, sigma2)):
        raise ValueError("frechet_distance: the moments hold values that are not finite")
    dev = sigma1.device
    ws = torch.empty(H.lib().mmvae_frechet_ws_doubles(F), dtype=torch.float64, device=dev)
    out = torch.empty(5, dtype=torch.float64, device=dev)
    sweeps = (ctypes.c_int * 2)()
    _call("mmvae_frechet_distance", H.ptr(mu1), H.ptr(sigma1), H.ptr(mu2), H.ptr(sigma2), H.ptr(ws), H.ptr(out), sweeps, F,
          H.stream())
    return {"distance": out[0], "tr_covmean": out[1], "sweeps": (sweeps[0], sweeps[1])}


# ---- k-nearest-neighbour manifold estimates of feature sets (csrc/manifold.hip): float64 distances, forward only ------------
def _manifold_k(who, k):
    k = int(k)
    if not 1 <= k <= H.MANIFOLD_MAX_K:
        raise ValueError(f"{who}: k = {k} neighbours (1 .. {H.MANIFOLD_MAX_K} are on the MI355X path)")
    return k


def _manifold_rows(who, what, X, least=1):
    return _feature_rows(who, what, X, least, H.MANIFOLD_MAX_ROWS, f"{least} .. {H.MANIFOLD_MAX_ROWS} are on the MI355X "
                                                                     f"path; the k-th neighbour needs k + 1 rows")


def _manifold_sqnorms(X):
    n2 = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
    _call("mmvae_manifold_sqnorms", H.ptr(X), H.ptr(n2), X.shape[0], X.shape[1], H.stream())
    return n2


def _manifold_radii(X, n2, k, chunks):
    N, F = X.shape
    ws = torch.empty(H.lib().mmvae_manifold_ws_doubles(N, N, k, chunks), dtype=torch.float64, device=X.device)
    rad2 = torch.empty(N, dtype=torch.float64, device=X.device)
    _call("mmvae_manifold_radii", H.ptr(X), H.ptr(n2), H.ptr(ws), H.ptr(rad2), N, F, k, chunks, H.stream())
    return rad2


def _manifold_cross(B, nb, A, na, rad2, chunks):
    (Nb, F), Na = B.shape, A.shape[0]
    ws = torch.empty(H.lib().mmvae_manifold_ws_doubles(Nb, Na, 1, chunks), dtype=torch.float64, device=B.device)
    count = torch.empty(Nb, dtype=torch.int32, device=B.device)
    mind2 = torch.empty(Nb, dtype=torch.float64, device=B.device)
    _call("mmvae_manifold_cross", H.ptr(B), H.ptr(nb), H.ptr(A), H.ptr(na), H.ptr(rad2), H.ptr(ws), H.ptr(count),
          H.ptr(mind2), Nb, Na, F, chunks, H.stream())
    return count, mind2


def manifold_sqnorms(X):
    """-> (N,) float64: |x_i|^2 of the fp32 rows, summed in double in feature order"""
    return _manifold_sqnorms(_manifold_rows("manifold_sqnorms", "X", X))


def manifold_radii(X, k, chunks=0):
    """-> (N,) float64: rad^2[i] = the k-th smallest squared distance from row i of X (N,F) to the other rows, the row itself
    left out by index (a duplicate row is a neighbour at distance 0).  d^2 = max(0, (|x|^2 + |y|^2) - 2 x . y) in double, the
    Gram product on the fp64 MFMA; the N x N matrix is never written.  `chunks`: how many workgroups share a row's columns
    (0: the default plan); the result does not depend on it, bit for bit."""
    k, chunks = _manifold_k("manifold_radii", k), _chunks("manifold_radii", chunks)
    X = _manifold_rows("manifold_radii", "X", X, least=k + 1)
    return _manifold_radii(X, _manifold_sqnorms(X), k, chunks)


def _manifold_rad2(who, rad2, A):
    if not torch.is_tensor(rad2) or tuple(rad2.shape) != (A.shape[0],) or rad2.dtype != torch.float64:
        said = f"{tuple(rad2.shape)}, {rad2.dtype}" if torch.is_tensor(rad2) else type(rad2).__name__
        raise ValueError(f"{who}: rad2 is {said}; float64 ({A.shape[0]},), one squared radius per manifold row")
    if rad2.device != A.device:
        raise ValueError(f"{who}: rad2 is on {rad2.device}, the manifold rows on {A.device}")
    rad2 = rad2.detach().contiguous()
    if bool(torch.isnan(rad2).any()):
        raise ValueError(f"{who}: rad2 holds NaN")
    return rad2


def manifold_cross(queries, manifold, rad2, chunks=0):
    """query rows (Nq,F) against manifold rows (Na,F) with their squared radii rad2 (Na,) float64
    -> (count (Nq,) int32 = the number of manifold rows whose sphere holds the query, d^2 <= rad^2: a point on a sphere is
        inside; mind2 (Nq,) float64 = the query's smallest squared distance to the manifold rows)."""
    chunks = _chunks("manifold_cross", chunks)
    B = _manifold_rows("manifold_cross", "queries", queries)
    A = _manifold_rows("manifold_cross", "manifold", manifold)
    if A.shape[1] != B.shape[1]:
        raise ValueError(f"manifold_cross: queries have F = {B.shape[1]} features, the manifold F = {A.shape[1]}")
    if A.device != B.device:
        raise ValueError(f"manifold_cross: the queries are on {B.device}, the manifold rows on {A.device}")
    rad2 = _manifold_rad2("manifold_cross", rad2, A)
    return _manifold_cross(B, _manifold_sqnorms(B), A, _manifold_sqnorms(A), rad2, chunks)


def manifold_prdc(real, fake, k=5, chunks=0):
    """Improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) of generated
    feature rows `fake` (M,F) against `real` (N,F), k-nearest-neighbour spheres, `<=` throughout:
      rad2_real, rad2_fake   manifold_radii of each set;
      hit_real[j]  = #{i : d^2(fake_j, real_i) <= rad2_real[i]},  hit_fake[i] = #{j : d^2(real_i, fake_j) <= rad2_fake[j]},
      near_real[i] = min_j d^2(real_i, fake_j);
      precision = mean_j [hit_real[j] > 0], recall = mean_i [hit_fake[i] > 0], density = sum_j hit_real[j] / (k M),
      coverage = mean_i [near_real[i] <= rad2_real[i]].
    -> the four as floats (quotients of integer sums: exact counts) and the five per-row tensors on the device."""
    k, chunks = _manifold_k("manifold_prdc", k), _chunks("manifold_prdc", chunks)
    R = _manifold_rows("manifold_prdc", "real", real, least=k + 1)
    G = _manifold_rows("manifold_prdc", "fake", fake, least=k + 1)
    if R.shape[1] != G.shape[1]:
        raise ValueError(f"manifold_prdc: real has F = {R.shape[1]} features, fake F = {G.shape[1]}")
    if R.device != G.device:
        raise ValueError(f"manifold_prdc: real is on {R.device}, fake on {G.device}")
    nr, ng = _manifold_sqnorms(R), _manifold_sqnorms(G)
    rad_r, rad_g = _manifold_radii(R, nr, k, chunks), _manifold_radii(G, ng, k, chunks)
    hit_r, _ = _manifold_cross(G, ng, R, nr, rad_r, chunks)
    hit_g, near_r = _manifold_cross(R, nr, G, ng, rad_g, chunks)
    N, M = R.shape[0], G.shape[0]
    return {"precision": int((hit_r > 0).sum()) / M, "recall": int((hit_g > 0).sum()) / N,
            "density": int(hit_r.sum(dtype=torch.int64)) / (k * M), "coverage": int((near_r <= rad_r).sum()) / N,
            "hit_real": hit_r, "hit_fake": hit_g, "near_real": near_r, "rad2_real": rad_r, "rad2_fake": rad_g}


# ---- kernel inception distance of feature sets (csrc/kid.hip): float64 sums of polynomial kernel values, forward only -------
def _kid_index(who, what, idx, rows, device):
    """contiguous int32 (S, m) on `device` or ValueError: an integer (S, m) tensor inside the limits, every entry in
    [0, rows) -- one min/max read on the device, before any C call: the kernel does not check"""
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        said = f"{tuple(idx.shape)}, {idx.dtype}" if torch.is_tensor(idx) else type(idx).__name__
        raise ValueError(f"{who}: {what} is {said}; an integer (S, m) tensor, one row of row numbers per subset")
    S, m = idx.shape
    if not 1 <= S <= H.KID_MAX_SUBSETS or not 2 <= m <= H.KID_MAX_SUBSET:
        raise ValueError(f"{who}: {what} is {S} subsets of m = {m} rows (1 .. {H.KID_MAX_SUBSETS} subsets of 2 .. "
                         f"{H.KID_MAX_SUBSET} rows are on the MI355X path)")
    if idx.device != device:
        raise ValueError(f"{who}: {what} is on {idx.device}, the features on {device}")
    idx = idx.detach()
    lo, hi = (int(v) for v in torch.aminmax(idx))
    if lo < 0 or hi >= rows:
        raise ValueError(f"{who}: {what} holds row numbers from {lo} to {hi}; the set has the rows 0 .. {rows - 1}")
    return idx.to(torch.int32).contiguous()


def _kid_kernel(who, F, degree, gamma, coef0, chunks):
    degree = int(degree)
    if not 1 <= degree <= H.KID_MAX_DEGREE:
        raise ValueError(f"{who}: degree = {degree} (1 .. {H.KID_MAX_DEGREE} are on the MI355X path)")
    chunks = _chunks(who, chunks)
    gamma, coef0 = 1.0 / F if gamma is None else float(gamma), float(coef0)
    if not math.isfinite(gamma) or not math.isfinite(coef0):
        raise ValueError(f"{who}: gamma = {gamma}, coef0 = {coef0} (finite numbers)")
    return degree, gamma, coef0, chunks


def _kid_sums(who, names, X, Y, idx_x, idx_y, degree, gamma, coef0, chunks):
    """every check of kid_sums, then the C call -> (sums, the int32 index lists handed to it)"""
    (nx, ny), (nix, niy) = names
    X, Y = (_feature_rows(who, what, t, 1, 2 ** 31 - 1, "1 .. 2^31 - 1: the index lists are int32", finite=False)
            for what, t in ((nx, X), (ny, Y)))      # (finite values: after the comparisons of the two sets)
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"{who}: {nx} has F = {X.shape[1]} features, {ny} F = {Y.shape[1]}")
    if X.device != Y.device:
        raise ValueError(f"{who}: {nx} is on {X.device}, {ny} on {Y.device}")
    _finite(who, nx, X)
    _finite(who, ny, Y)
    F = X.shape[1]
    degree, gamma, coef0, chunks = _kid_kernel(who, F, degree, gamma, coef0, chunks)
    if torch.is_tensor(idx_x) and torch.is_tensor(idx_y) and idx_x.shape != idx_y.shape:
        raise ValueError(f"{who}: {nix} is {tuple(idx_x.shape)}, {niy} {tuple(idx_y.shape)}; both (S, m)")
    idx_x = _kid_index(who, nix, idx_x, X.shape[0], X.device)
    idx_y = _kid_index(who, niy, idx_y, Y.shape[0], X.device)
    if X.device.type != "cuda":
        raise ValueError(f"{who}: {nx} is on {X.device}; the kernel runs on the MI355X (there is no host path)")
    S, m = idx_x.shape
    ws = torch.empty(H.lib().mmvae_kid_ws_doubles(S, m, chunks), dtype=torch.float64, device=X.device)
    sums = torch.empty(S, 3, dtype=torch.float64, device=X.device)
    _call("mmvae_kid_sums", H.ptr(X), H.ptr(Y), H.ptr(idx_x), H.ptr(idx_y), H.ptr(ws), H.ptr(sums), X.shape[0], Y.shape[0],
          F, S, m, degree, gamma, coef0, chunks, H.stream())
    return sums, idx_x, idx_y


def kid_sums(X, Y, idx_x, idx_y, degree=3, gamma=None, coef0=1.0, chunks=0):
    """The sums behind the kernel inception distance: feature rows X (rows_x,F), Y (rows_y,F); idx_x, idx_y integer (S,m),
    per subset the rows taken from X and from Y.  With k(x, y) = (gamma x . y + coef0)^degree (gamma None: 1 / F),
    x_i = X[idx_x[s,i]], y_j = Y[idx_y[s,j]] -> (S,3) float64 = [sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j),
    sum_{i,j} k(x_i, y_j)], the diagonal of the first two left out by position in the list.  Dot products in double on the
    fp64 MFMA, the rows gathered through the lists as they are loaded; neither a gathered copy nor an m x m block is
    written.  `chunks`: how many workgroups share a row's columns (0: the default plan); two plans regroup fp64 sums
    (agreement to rounding, not bit for bit), two runs with one plan give the same bits.  Every index is checked to lie
    inside its set (one min/max read per list) before the kernel runs."""
    return _kid_sums("kid_sums", (("X", "Y"), ("idx_x", "idx_y")), X, Y, idx_x, idx_y, degree, gamma, coef0, chunks)[0]


def kid_draw(n_real, n_fake, subsets, m, seed):
    """the subsets of a kernel inception distance, drawn on the host: rs = numpy.random.RandomState(seed); for s in order
    rs.choice(n_real, m, replace=False), then rs.choice(n_fake, m, replace=False) -> two (subsets, m) int64 arrays"""
    rs = np.random.RandomState(seed)
    idx_real, idx_fake = np.empty((subsets, m), dtype=np.int64), np.empty((subsets, m), dtype=np.int64)
    for s in range(subsets):
        idx_real[s] = rs.choice(n_real, m, replace=False)
        idx_fake[s] = rs.choice(n_fake, m, replace=False)
    return idx_real, idx_fake


def kernel_inception_distance(real, fake, subsets=100, subset_size=1000, seed=0, idx=None, degree=3, gamma=None, coef0=1.0,
                              chunks=0):
    """Kernel inception distance (Binkowski et al. 2018) of generated feature rows `fake` (M,F) against `real` (N,F): the
    unbiased estimate of the squared maximum mean discrepancy under k(x, y) = (gamma x . y + coef0)^degree (gamma None:
    1 / F), over `subsets` random subsets of m = min(subset_size, N, M) rows of each set, drawn without replacement
    (kid_draw(N, M, subsets, m, seed)) or given as idx = (idx_real, idx_fake), integer (S, m):
      mmd2[s] = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2,   (sxx, syy, sxy) = kid_sums(...)[s]
    -> {"kid": mean_s mmd2, "std": the standard deviation of mmd2 over the subsets (divisor S), both float64 0-d tensors
        on the device, "mmd2": (S,), "sums": (S,3), "idx_real", "idx_fake": (S,m) int32 on the device, "m": m}.
    The estimator is unbiased: a negative mmd2 (and kid) is a legitimate value and is not clamped."""
    who = "kernel_inception_distance"
    if idx is None:
        if not all(torch.is_tensor(t) and t.dim() == 2 for t in (real, fake)):
            raise ValueError(f"{who}: real and fake are floating (rows, F) features")
        subsets, m = int(subsets), min(int(subset_size), real.shape[0], fake.shape[0])
        if m < 2:
            raise ValueError(f"{who}: m = min(subset_size = {subset_size}, {real.shape[0]} real rows, {fake.shape[0]} "
                             f"generated rows) = {m} (the unbiased estimate needs two rows of each set)")
        if not 1 <= subsets <= H.KID_MAX_SUBSETS or m > H.KID_MAX_SUBSET:
            raise ValueError(f"{who}: {subsets} subsets of m = {m} rows (1 .. {H.KID_MAX_SUBSETS} subsets of 2 .. "
                             f"{H.KID_MAX_SUBSET} rows are on the MI355X path)")
        idx = tuple(torch.from_numpy(i).to(device=real.device, dtype=torch.int32)
                    for i in kid_draw(real.shape[0], fake.shape[0], subsets, m, seed))
    elif not isinstance(idx, (tuple, list)) or len(idx) != 2:
        raise ValueError(f"{who}: idx is (idx_real, idx_fake), two integer (S, m) tensors")
    sums, idx_real, idx_fake = _kid_sums(who, (("real", "fake"), ("idx_real", "idx_fake")), real, fake, idx[0], idx[1],
                                         degree, gamma, coef0, chunks)
    m = idx_real.shape[1]
    mmd2 = sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)
    return {"kid": mmd2.mean(), "std": mmd2.std(unbiased=False), "mmd2": mmd2, "sums": sums, "idx_real": idx_real,
            "idx_fake": idx_fake, "m": m}


# ---- latent cluster analysis (csrc/cluster.hip): k-means, partition statistics, silhouette; float64, forward only -----------
KMEANS_CHECK_EVERY = 8      # iterations per enqueued call and between two looks at the restarts' states


def _cluster_rows(who, X):
    return _feature_rows(who, "X", X, 1, H.MANIFOLD_MAX_ROWS, f"1 .. {H.MANIFOLD_MAX_ROWS} are on the MI355X path")


def _cluster_count(who, C, N):
    C = int(C)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} clusters (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if C > N:
        raise ValueError(f"{who}: {C} clusters for {N} rows (at most one cluster per row on the MI355X path)")
    return C


def _cluster_labels(who, what, labels, N, device=None):
    """an integer (N,) tensor (N None: of any length >= 1) of ids >= 0 (on `device`, where one is given) or ValueError
    -> (labels, the largest id)"""
    if isinstance(labels, (np.ndarray, list, tuple)):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.numel() == 0 or labels.is_floating_point() or labels.is_complex() or \
            labels.dtype == torch.bool:
        said = f"{tuple(labels.shape)}, {labels.dtype}" if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"{who}: {what} is {said}; an integer (N,) tensor, one cluster id per row")
    if N is not None and labels.shape[0] != N:
        raise ValueError(f"{who}: {what} has {labels.shape[0]} entries for {N} rows")
    if device is not None and labels.device != device:
        raise ValueError(f"{who}: {what} is on {labels.device}, the rows on {device}")
    labels = labels.detach()
    lo, hi = (int(v) for v in torch.aminmax(labels))
    if lo < 0:
        raise ValueError(f"{who}: {what} holds negative ids (clusters are numbered from 0)")
    return labels, hi


def _cluster_partition(who, X, labels, n_clusters):
    """the checks shared by cluster_stats and silhouette -> (X fp32, labels int32 on its device, C)"""
    X = _cluster_rows(who, X)
    labels, hi = _cluster_labels(who, "labels", labels, X.shape[0], X.device)
    C = hi + 1 if n_clusters is None else int(n_clusters)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} clusters (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if hi >= C:
        raise ValueError(f"{who}: labels holds the id {hi}; n_clusters = {C} has the ids 0 .. {C - 1}")
    return X, labels.to(torch.int32).contiguous(), C


def _need_device(who, X):
    if X.device.type != "cuda":
        raise ValueError(f"{who}: X is on {X.device}; the kernels run on the MI355X (there is no host path)")


def kmeans_draw(N, C, n_init, seed):
    """the start centres of a k-means fit, drawn on the host: rs = numpy.random.RandomState(seed); per restart, in order,
    rs.permutation(N)[:C] -> (n_init, C) int32 row numbers, no row twice within a restart"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(N)[:C] for _ in range(n_init)]).astype(np.int32)


def _cluster_spread(labels, d2, C):
    R, N = labels.shape
    counts = torch.empty(R, C, dtype=torch.int32, device=labels.device)
    within, wdist = (torch.empty(R, C, dtype=torch.float64, device=labels.device) for _ in range(2))
    inertia = torch.empty(R, dtype=torch.float64, device=labels.device)
    _call("mmvae_cluster_spread", H.ptr(labels), H.ptr(d2), H.ptr(counts), H.ptr(within), H.ptr(wdist), H.ptr(inertia), N, C,
          R, H.stream())
    return counts, within, wdist, inertia


def kmeans_check_init(who, init, N, F, C=None):
    """the start centres of a k-means fit on (N, F) rows or ValueError: integer (R, C) row numbers inside [0, N), none twice
    within a restart, or finite float64 (R, C, F) centres; R, C inside the limits, C <= N (and equal to `C`, where given)
    -> (init as a tensor, whether it holds row numbers)"""
    if isinstance(init, np.ndarray):
        init = torch.from_numpy(np.ascontiguousarray(init))
    rows = torch.is_tensor(init) and init.dim() == 2 and not init.is_floating_point() and not init.is_complex() and \
        init.dtype != torch.bool
    if not rows and not (torch.is_tensor(init) and init.dim() == 3 and init.dtype == torch.float64):
        said = f"{tuple(init.shape)}, {init.dtype}" if torch.is_tensor(init) else type(init).__name__
        raise ValueError(f"{who}: init is {said}; integer (R, C) row numbers or float64 (R, C, F) centres")
    if not 1 <= init.shape[0] <= H.CLUSTER_MAX_INIT:
        raise ValueError(f"{who}: {init.shape[0]} restarts (1 .. {H.CLUSTER_MAX_INIT} are on the MI355X path)")
    if _cluster_count(who, init.shape[1], N) != (init.shape[1] if C is None else C):
        raise ValueError(f"{who}: init holds {init.shape[1]} centres per restart, n_clusters = {C}")
    init = init.detach()
    if rows:
        lo, hi = (int(v) for v in torch.aminmax(init))
        if lo < 0 or hi >= N:
            raise ValueError(f"{who}: init holds row numbers from {lo} to {hi}; X has the rows 0 .. {N - 1}")
        ordered = torch.sort(init.long(), dim=1).values
        if bool((ordered[:, 1:] == ordered[:, :-1]).any()):
            raise ValueError(f"{who}: init names a row twice within one restart (two equal start centres)")
    else:
        if init.shape[2] != F:
            raise ValueError(f"{who}: init has centres of {init.shape[2]} features, X F = {F}")
        _finite(who, "init", init)
    return init, rows


def kmeans_fit(X, init, max_iter=300):
    """k-means (Lloyd) on the rows of X (N,F), read as double, from given start centres, R restarts side by side.
    `init`: integer (R,C) row numbers (centre c of restart r starts as row init[r, c]; kmeans_draw) or float64 (R,C,F)
    centres.  Per restart, iteration t = 1, 2, ...: labels = the nearest centre by d^2 = sum_f (x_f - mu_f)^2 (a tie goes
    to the lowest index); t > 1 and no label changed: converged, n_iter = t; else every centre becomes the mean of its rows
    (summed in index order; a cluster without rows keeps its centre and counts in `empty`); after `max_iter` updates
    without convergence one more assignment gives the labels of the returned centres.  This is scikit-learn's
    KMeans(init=<array>, n_init=1, tol=0, algorithm="lloyd") on float64 input, except that it relocates empty clusters.
    Two launches per iteration for all restarts; the host reads the restarts' states every KMEANS_CHECK_EVERY iterations.
    -> {"centres" (R,C,F) float64, "labels" (R,N) int32, "inertia" (R,) float64 = sum_i d^2[i, label_i], "n_iter" (R,) int32,
        "converged" (R,) bool, "empty" (R,) int32, "counts" (R,C) int32, "best": the restart of the smallest inertia (the
        lowest of equals)}.  Two runs, and a restart alone or beside others, give the same bits."""
    who = "kmeans_fit"
    X = _cluster_rows(who, X)
    N, F = X.shape
    max_iter = int(max_iter)
    if not 1 <= max_iter <= H.CLUSTER_MAX_ITER:
        raise ValueError(f"{who}: max_iter = {max_iter} (1 .. {H.CLUSTER_MAX_ITER} are on the MI355X path)")
    init, rows = kmeans_check_init(who, init, N, F)
    R, C = init.shape[:2]
    init = init.to(X.device)
    _need_device(who, X)
    centres = (X.double()[init.long()] if rows else init.clone()).contiguous()
    labels = torch.zeros(R, N, dtype=torch.int32, device=X.device)
    ws = torch.zeros(H.lib().mmvae_cluster_lloyd_ws_ints(N, R), dtype=torch.int32, device=X.device)
    state = ws[:4 * R].view(R, 4)
    for it0 in range(1, max_iter + 1, KMEANS_CHECK_EVERY):
        _call("mmvae_cluster_lloyd", H.ptr(X), H.ptr(centres), H.ptr(labels), H.ptr(ws), N, F, C, R, it0,
              min(KMEANS_CHECK_EVERY, max_iter - it0 + 1), max_iter, H.stream())
        if bool((state[:, 0] != 0).all()):
            break
    d2 = torch.empty(R, N, dtype=torch.float64, device=X.device)
    _call("mmvae_cluster_assign", H.ptr(X), H.ptr(centres), H.ptr(labels), H.ptr(d2), N, F, C, R, 0, H.stream())
    counts, _, _, inertia = _cluster_spread(labels, d2, C)
    state = state.clone()
    finished = state[:, 0] != 0
    empties = ws[ws.numel() - R * H.CLUSTER_MAX_K:].view(R, H.CLUSTER_MAX_K)      # (per cluster: the updates it had no rows at)
    return {"centres": centres, "labels": labels, "inertia": inertia,
            "n_iter": torch.where(finished, state[:, 1], torch.full_like(state[:, 1], max_iter)),
            "converged": finished & (state[:, 2] != 0), "empty": empties.sum(1).to(torch.int32), "counts": counts,
            "best": int(np.argmin(inertia.cpu().numpy()))}


def cluster_stats(X, labels, n_clusters):
    """The statistics of the partition `labels` (N,) of the rows of X (N,F) into the ids 0 .. n_clusters - 1, in double:
    -> {"counts" (C,) int32, "means" (C,F) float64 (the rows summed in index order; 0 for an id without rows), "within" (C,)
        = sum_{i in c} |x_i - m_c|^2, "wdist" (C,) = sum_{i in c} |x_i - m_c|, rows in index order}."""
    who = "cluster_stats"
    if n_clusters is None:
        raise ValueError(f"{who}: n_clusters is None (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    X, labels, C = _cluster_partition(who, X, labels, n_clusters)
    _need_device(who, X)
    N, F = X.shape
    labels = labels.view(1, N)
    means = torch.zeros(1, C, F, dtype=torch.float64, device=X.device)
    counts = torch.empty(1, C, dtype=torch.int32, device=X.device)
    d2 = torch.empty(1, N, dtype=torch.float64, device=X.device)
    _call("mmvae_cluster_means", H.ptr(X), H.ptr(labels), H.ptr(means), H.ptr(counts), N, F, C, 1, H.stream())
    _call("mmvae_cluster_assign", H.ptr(X), H.ptr(means), H.ptr(labels), H.ptr(d2), N, F, C, 1, 1, H.stream())
    counts, within, wdist, _ = _cluster_spread(labels, d2, C)
    return {"counts": counts[0], "means": means[0], "within": within[0], "wdist": wdist[0]}


def cluster_indices(stats):
    """Calinski-Harabasz and Davies-Bouldin indices from cluster_stats' result, on the host in float64 as scikit-learn's
    calinski_harabasz_score and davies_bouldin_score compute them, over the C' clusters that have rows:
      CH = [sum_c n_c |m_c - m|^2 / (C' - 1)] / [sum_c within_c / (N - C')], m the mean of all rows (1 where the clusters
      have no spread); DB = mean_c max_{c' != c} (wdist_c / n_c + wdist_c' / n_c') / |m_c - m_c'| (0 where every spread or
      every distance between means vanishes).  -> {"calinski_harabasz": float, "davies_bouldin": float}"""
    who = "cluster_indices"
    if not isinstance(stats, dict) or any(k not in stats for k in ("counts", "means", "within", "wdist")):
        raise ValueError(f"{who}: stats is what cluster_stats returns (counts, means, within, wdist)")
    n_all, m, within, wdist = (np.asarray(torch.as_tensor(stats[k]).detach().cpu().numpy())
                               for k in ("counts", "means", "within", "wdist"))
    if m.ndim != 2 or any(v.shape != (m.shape[0],) for v in (n_all, within, wdist)):
        raise ValueError(f"{who}: stats holds counts, within, wdist (C,) and means (C, F)")
    on = n_all > 0
    n, m, within, wdist = n_all[on].astype(np.float64), m[on].astype(np.float64), within[on], wdist[on]
    N, C = n.sum(), len(n)
    if not 2 <= C < N:
        raise ValueError(f"{who}: {C} clusters with rows for {int(N)} rows (the indices need 2 .. N - 1)")
    mean = (n[:, None] * m).sum(0) / N
    extra, intra = float((n * ((m - mean) ** 2).sum(1)).sum()), float(within.sum())
    ch = 1.0 if intra == 0.0 else extra * (N - C) / (intra * (C - 1.0))
    spread = wdist / n
    between = np.sqrt(((m[:, None, :] - m[None, :, :]) ** 2).sum(2))
    if np.allclose(spread, 0) or np.allclose(between, 0):
        db = 0.0
    else:
        between[between == 0] = np.inf
        db = float(np.mean(np.max((spread[:, None] + spread[None, :]) / between, axis=1)))
    return {"calinski_harabasz": float(ch), "davies_bouldin": db}


def _silhouette_plan(counts, N, chunks):
    """the padded column list's layout and the chunk table from the clusters' sizes (host) -> (tile offset per cluster,
    padded length, table (chunks, 3) int32 = (cluster, first tile, tile past the last), first (C + 1,) int32)"""
    tiles = (counts + 63) // 64
    offset = np.concatenate(([0], np.cumsum(tiles)))
    per = H.lib().mmvae_cluster_sil_tiles_per_chunk(N, int(offset[-1]), chunks)
    table, first = [], [0]
    for c, t in enumerate(tiles):
        table += [(c, int(offset[c]) + t0, int(offset[c]) + min(t0 + per, int(t))) for t0 in range(0, int(t), per)]
        first.append(len(table))
    return offset, 64 * int(offset[-1]), np.array(table, dtype=np.int32).reshape(-1, 3), np.array(first, dtype=np.int32)


def silhouette(X, labels, n_clusters=None, chunks=0):
    """Silhouette of the partition `labels` (N,) of the rows of X (N,F); ids 0 .. n_clusters - 1 (None: the largest id + 1),
    ids without rows allowed.  d(i, j) = sqrt(max(0, (|x_i|^2 + |x_j|^2) - 2 x_i . x_j)) in double, the product on the fp64
    MFMA; S[i, c] = sum_{j in c, j != i} d(i, j), the row itself left out by INDEX (a duplicate row is an ordinary member
    at distance 0); a = S[i, l_i] / (n_l - 1), b = min over the other clusters with rows of S[i, c] / n_c,
    s_i = (b - a) / max(a, b), 0 in a cluster of one row and where max(a, b) = 0.  Neither the N x N matrix nor an N x n_c
    block is written: the columns are walked through a list of row numbers sorted by cluster.  `chunks`: 0 = the default
    plan, or the number of chunks the column list is cut into before the cuts at the cluster borders; two plans regroup
    fp64 sums (agreement to rounding), two runs with one plan give the same bits.
    -> {"samples" (N,) float64, "score": float = mean_i s_i, "sums" S (N,C) float64, "counts" (C,) int64}."""
    who = "silhouette"
    X, labels, C = _cluster_partition(who, X, labels, n_clusters)
    chunks = _chunks(who, chunks)
    N, F = X.shape
    lab = labels.long()
    cnt = torch.bincount(lab, minlength=C)
    counts = cnt.cpu().numpy()
    if int((counts > 0).sum()) < 2:
        raise ValueError(f"{who}: labels puts every row into one cluster (the silhouette needs two clusters with rows)")
    _need_device(who, X)
    dev = X.device
    offset, padded, table, first = _silhouette_plan(counts, N, chunks)
    order = torch.argsort(lab, stable=True)
    of = lab[order]
    start = torch.from_numpy(np.concatenate(([0], np.cumsum(counts)[:-1]))).to(dev)
    place = 64 * torch.from_numpy(offset[:-1]).to(dev)[of] + (torch.arange(N, device=dev) - start[of])
    column_list = torch.full((padded,), -1, dtype=torch.int32, device=dev)
    column_list[place] = order.to(torch.int32)
    n_chunks = len(table)
    ws = torch.empty(H.lib().mmvae_cluster_sil_ws_doubles(N, n_chunks), dtype=torch.float64, device=dev)
    S = torch.empty(N, C, dtype=torch.float64, device=dev)
    n2, table, first = _manifold_sqnorms(X), torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev)
    _call("mmvae_cluster_sil_sums", H.ptr(X), H.ptr(n2), H.ptr(column_list), H.ptr(table), H.ptr(first), H.ptr(ws), H.ptr(S),
          N, F, C, padded, n_chunks, H.stream())
    own = cnt[lab]
    a = S.gather(1, lab[:, None])[:, 0] / (own - 1).clamp(min=1)
    others = (cnt[None, :] > 0) & (torch.arange(C, device=dev)[None, :] != lab[:, None])
    b = torch.where(others, S / cnt.clamp(min=1)[None, :], torch.full_like(S, float("inf"))).min(1).values
    top = torch.maximum(a, b)
    s = torch.where((own > 1) & (top > 0), (b - a) / top, torch.zeros_like(top))
    return {"samples": s, "score": float(s.mean()), "sums": S, "counts": cnt}


def cluster_agreement(a, b):
    """Agreement of two labelings of the same rows, a the classes and b the clusters, from their integer contingency table
    T[class, cluster] on the host in float64, as scikit-learn defines them: adjusted Rand index, normalised mutual
    information (arithmetic mean of the entropies, natural logarithm), homogeneity, completeness, and purity = sum over
    the clusters of max_class T / N.  -> {"ari", "nmi", "homogeneity", "completeness", "purity"}: floats"""
    who = "cluster_agreement"
    sides = []
    for what, t in (("a", a), ("b", b)):
        sides.append(_cluster_labels(who, what, t, None)[0].cpu().numpy())
    if len(sides[0]) != len(sides[1]):
        raise ValueError(f"{who}: a has {len(sides[0])} entries, b {len(sides[1])} (one pair of ids per row)")
    ia, ib = (np.unique(t, return_inverse=True)[1] for t in sides)
    T = np.zeros((int(ia.max()) + 1, int(ib.max()) + 1), dtype=np.int64)
    np.add.at(T, (ia, ib), 1)
    N, ra, rb = int(T.sum()), T.sum(1), T.sum(0)
    sq = int((T * T).sum())
    tp, fp, fn = sq - N, int((T @ rb).sum()) - sq, int((T.T @ ra).sum()) - sq
    tn = N * N - fp - fn - sq
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    i, j = np.nonzero(T)
    v = T[i, j].astype(np.float64)
    mi = float(max(np.sum(v / N * (np.log(v) - math.log(N)) + v / N * (-np.log(ra[i] * rb[j].astype(np.float64))
                                                                       + 2.0 * math.log(N))), 0.0))

    def entropy(n):
        n = n[n > 0].astype(np.float64)
        return float(-np.sum((n / n.sum()) * (np.log(n) - math.log(n.sum()))))
    ha, hb, tiny = entropy(ra), entropy(rb), float(np.finfo(np.float64).eps)
    if len(ra) == 1 and len(rb) == 1:
        nmi = 1.0
    else:
        nmi = 0.0 if mi <= tiny else mi / max(0.5 * (ha + hb), tiny)
    return {"ari": float(ari), "nmi": float(nmi), "homogeneity": mi / ha if ha else 1.0,
            "completeness": mi / hb if hb else 1.0, "purity": float(T.max(0).sum()) / N}


# ---- latent density estimation (csrc/gmm.hip): Gaussian-mixture EM, scoring, draws; float64, forward only --------------------
GMM_SLICE_BYTES = 256 << 20      # restarts run in slices whose responsibilities and workspace stay under this


def _gmm_rows(who, X, D=None):
    """contiguous fp32 (N, D) rows inside the limits (and of `D` dimensions, where given) or ValueError"""
    X = _feature_rows(who, "X", X, 1, H.MANIFOLD_MAX_ROWS, f"1 .. {H.MANIFOLD_MAX_ROWS} are on the MI355X path", finite=False)
    if not 1 <= X.shape[1] <= H.GMM_MAX_D:
        raise ValueError(f"{who}: X has D = {X.shape[1]} dimensions (1 .. {H.GMM_MAX_D} are on the MI355X path)")
    if D is not None and X.shape[1] != D:
        raise ValueError(f"{who}: X has D = {X.shape[1]} dimensions, the mixture {D}")
    _finite(who, "X", X)
    return X


def _gmm_covariance(who, covariance_type):
    if covariance_type not in H.GMM_COVARIANCES:
        raise ValueError(f"{who}: covariance_type = {covariance_type!r} ({', '.join(map(repr, H.GMM_COVARIANCES))} are on "
                         f"the MI355X path)")
    return H.GMM_COVARIANCES[covariance_type]


def gmm_check_init(who, init, N, n_components=None):
    """the start of a mixture fit on N rows or ValueError: integer (R, N) labels, one per row and restart, inside
    [0, n_components) (None: the largest id + 1 components); R and the components inside the limits
    -> (init as an int32 tensor, C)"""
    if isinstance(init, np.ndarray):
        init = torch.from_numpy(np.ascontiguousarray(init))
    if not torch.is_tensor(init) or init.dim() != 2 or init.is_floating_point() or init.is_complex() or init.dtype == torch.bool:
        said = f"{tuple(init.shape)}, {init.dtype}" if torch.is_tensor(init) else type(init).__name__
        raise ValueError(f"{who}: init is {said}; integer (R, N) labels, one component id per restart and row")
    if not 1 <= init.shape[0] <= H.CLUSTER_MAX_INIT:
        raise ValueError(f"{who}: {init.shape[0]} restarts (1 .. {H.CLUSTER_MAX_INIT} are on the MI355X path)")
    if init.shape[1] != N:
        raise ValueError(f"{who}: init has {init.shape[1]} labels per restart for {N} rows")
    init = init.detach()
    lo, hi = (int(v) for v in torch.aminmax(init))
    C = hi + 1 if n_components is None else int(n_components)
    if not 1 <= C <= H.CLUSTER_MAX_K:
        raise ValueError(f"{who}: {C} components (1 .. {H.CLUSTER_MAX_K} are on the MI355X path)")
    if lo < 0 or hi >= C:
        raise ValueError(f"{who}: init holds the ids {lo} .. {hi}; n_components = {C} has the ids 0 .. {C - 1}")
    return init.to(torch.int32).contiguous(), C


def _gmm_fit_args(who, reg_covar, tol, max_iter):
    reg_covar, tol, max_iter = float(reg_covar), float(tol), int(max_iter)
    if not (reg_covar >= 0.0 and math.isfinite(reg_covar)):
        raise ValueError(f"{who}: reg_covar = {reg_covar} (a finite value >= 0)")
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"{who}: tol = {tol} (a finite value >= 0)")
    if not 1 <= max_iter <= H.CLUSTER_MAX_ITER:
        raise ValueError(f"{who}: max_iter = {max_iter} (1 .. {H.CLUSTER_MAX_ITER} are on the MI355X path)")
    return reg_covar, tol, max_iter


def gmm_fit(X, init, covariance_type="full", reg_covar=1e-6, tol=1e-3, max_iter=100, sync_every=10, n_components=None,
            slice_bytes=None):
    """EM for a mixture of C Gaussians on the rows of X (N,D), read as double, R restarts side by side, with the arithmetic of
    scikit-learn's GaussianMixture (covariance_type "full" or "diag").  `init`: integer (R,N) labels; restart r starts from
    their one-hot as responsibilities and one M-step (C = `n_components`, or the largest id + 1; a component without rows
    starts as N(0, reg_covar I) with weight ~0).  Iteration t = 1, 2, ...: E-step, M-step; the restart has converged when the
    E-step's lower bound (the mean log-density) moved by less than `tol`; n_iter = t.  A restart one of whose covariances
    has no Cholesky factor is `degenerate` (bound -inf, never `best`); when every restart is, ValueError.  Three launches
    per iteration for all restarts; the host reads the restarts' records every `sync_every` iterations.  Restarts run in
    slices of `slice_bytes` (GMM_SLICE_BYTES) of responsibilities and workspace.
    -> {"weights" (R,C), "means" (R,C,D), "covariances" (R,C,D,D) | (R,C,D), "cholesky" (lower factors; diag: square roots),
        "precisions_cholesky", "log_det" (R,C), "lower_bound" (R,), "n_iter" (R,) int32, "converged", "degenerate" (R,) bool,
        "best": the restart of the largest bound (the lowest of equals), "labels" (R,N) int32, "resp" (R,N,C), "log_density"
        (R,N) of the final parameters, "covariance_type"}, float64.  Two runs, a restart alone or beside others, any
        `sync_every` and any slicing give the same bits."""
    who = "gmm_fit"
    X = _gmm_rows(who, X)
    N, D = X.shape
    diag = _gmm_covariance(who, covariance_type)
    reg_covar, tol, max_iter = _gmm_fit_args(who, reg_covar, tol, max_iter)
    sync_every = int(sync_every)
    if sync_every < 1:
        raise ValueError(f"{who}: sync_every = {sync_every} (at least one iteration between two looks at the records)")
    init, C = gmm_check_init(who, init, N, n_components)
    R = init.shape[0]
    slice_bytes = GMM_SLICE_BYTES if slice_bytes is None else int(slice_bytes)
    if slice_bytes < 1:
        raise ValueError(f"{who}: slice_bytes = {slice_bytes} (a positive number of bytes; one restart runs in any case)")
    _need_device(who, X)
    dev = X.device
    init = init.to(dev)
    per = 8 * (N * C + H.lib().mmvae_gmm_ws_doubles(N, D, C, 1, diag))
    step = max(1, min(R, slice_bytes // per))
    shape = (D,) if diag else (D, D)
    parts = []
    for r0 in range(0, R, step):
        Rs = min(step, R - r0)
        f64 = dict(dtype=torch.float64, device=dev)
        weights, logdet = torch.empty(Rs, C, **f64), torch.empty(Rs, C, **f64)
        means = torch.empty(Rs, C, D, **f64)
        cov, chol, prec = (torch.empty(Rs, C, *shape, **f64) for _ in range(3))
        resp = torch.empty(Rs, N, C, **f64)
        ws = torch.zeros(H.lib().mmvae_gmm_ws_doubles(N, D, C, Rs, diag), **f64)
        state = ws[:4 * Rs].view(Rs, 4)
        bad = ws[4 * Rs:(4 + H.CLUSTER_MAX_K) * Rs].view(Rs, H.CLUSTER_MAX_K)
        start = init[r0:r0 + Rs].contiguous()
        for it0 in range(1, max_iter + 1, sync_every):
            _call("mmvae_gmm_em", H.ptr(X), H.ptr(start), H.ptr(weights), H.ptr(means), H.ptr(cov), H.ptr(chol), H.ptr(prec),
                  H.ptr(logdet), H.ptr(resp), H.ptr(ws), N, D, C, Rs, diag, reg_covar, tol, it0,
                  min(sync_every, max_iter - it0 + 1), max_iter, H.stream())
            if bool(((state[:, 3] != 0) | (bad != 0).any(1)).all()):
                break
        logdens = torch.empty(Rs, N, **f64)
        labels = torch.empty(Rs, N, dtype=torch.int32, device=dev)
        _call("mmvae_gmm_score", H.ptr(X), H.ptr(weights), H.ptr(means), H.ptr(prec), H.ptr(logdet), H.ptr(logdens),
              H.ptr(resp), H.ptr(labels), N, D, C, Rs, diag, H.stream())
        degenerate = (bad != 0).any(1)
        parts.append({"weights": weights, "means": means, "covariances": cov, "cholesky": chol, "precisions_cholesky": prec,
                      "log_det": logdet,
                      "lower_bound": torch.where(degenerate, torch.full_like(state[:, 0], -math.inf), state[:, 0]),
                      "n_iter": state[:, 1].to(torch.int32), "converged": (state[:, 2] != 0) & ~degenerate,
                      "degenerate": degenerate, "labels": labels, "resp": resp, "log_density": logdens})
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    bound = out["lower_bound"].cpu().numpy()
    if bool(out["degenerate"].all()):
        raise ValueError(f"{who}: every restart met a covariance without a Cholesky factor (a component of a single row or of "
                         f"equal rows); reg_covar = {reg_covar}: increase it, or ask for fewer components")
    out["best"] = int(np.argmax(bound))      # (degenerate restarts hold -inf; the first of equals)
    out["covariance_type"] = covariance_type
    return out


def _gmm_mixture(who, fit, restart):
    """one mixture out of what gmm_fit returns (`restart`, None: its best) or of a single mixture's entry (weights (C,), as
    TorchMMVAE.fit_latent_density returns per subset; `restart` must be None) or ValueError
    -> ({"weights" (C,), "means" (C,D), "cholesky", "precisions_cholesky", "log_det" (C,)}: contiguous float64, diag, restart)"""
    keys = ("weights", "means", "cholesky", "precisions_cholesky", "log_det")
    if not isinstance(fit, dict) or any(not torch.is_tensor(fit.get(k)) or fit[k].dtype != torch.float64 for k in keys) or \
            "covariance_type" not in fit:
        raise ValueError(f"{who}: fit is what gmm_fit returns (float64 {', '.join(keys)}; covariance_type)")
    diag = _gmm_covariance(who, fit["covariance_type"])
    many = fit["weights"].dim() == 2
    if many:
        R = fit["weights"].shape[0]
        restart = fit.get("best") if restart is None else restart
        if not isinstance(restart, (int, np.integer)) or not 0 <= restart < R:
            raise ValueError(f"{who}: restart = {restart!r} (the fit holds the restarts 0 .. {R - 1})")
        if "degenerate" in fit and bool(fit["degenerate"][restart]):
            raise ValueError(f"{who}: restart {restart} is degenerate (a covariance without a Cholesky factor)")
        restart = int(restart)
    elif restart is not None:
        raise ValueError(f"{who}: restart = {restart!r} for a single mixture (None)")
    m = {k: (fit[k][restart] if many else fit[k]).detach().contiguous() for k in keys}
    C = m["weights"].shape[0] if m["weights"].dim() == 1 else 0
    D = m["means"].shape[1] if m["means"].dim() == 2 else 0
    shape = (C, D) if diag else (C, D, D)
    if not 1 <= C <= H.CLUSTER_MAX_K or not 1 <= D <= H.GMM_MAX_D or m["means"].shape != (C, D) or m["log_det"].shape != (C,) or \
            m["cholesky"].shape != shape or m["precisions_cholesky"].shape != shape:
        raise ValueError(f"{who}: fit holds weights {tuple(m['weights'].shape)}, means {tuple(m['means'].shape)}, factors "
                         f"{tuple(m['cholesky'].shape)}; (C), (C, D) and {'(C, D)' if diag else '(C, D, D)'} with C <= "
                         f"{H.CLUSTER_MAX_K}, D <= {H.GMM_MAX_D} are on the MI355X path")
    return m, diag, restart


def gmm_score(X, fit, restart=None):
    """The log-density of the rows of X (N,D) under one mixture of `fit` (gmm_fit's result and a restart, None: its best; or a
    single mixture's entry), by the E-step's kernel: on the fitted rows it returns the fit's own bits.
    -> {"log_density" (N,) float64, "labels" (N,) int32 (the first most probable component), "resp" (N,C), "score": the mean}"""
    who = "gmm_score"
    m, diag, _ = _gmm_mixture(who, fit, restart)
    C, D = m["means"].shape
    X = _gmm_rows(who, X, D)
    N = X.shape[0]
    _need_device(who, X)
    m = {k: v.to(X.device) for k, v in m.items()}
    logdens = torch.empty(N, dtype=torch.float64, device=X.device)
    resp = torch.empty(N, C, dtype=torch.float64, device=X.device)
    labels = torch.empty(N, dtype=torch.int32, device=X.device)
    _call("mmvae_gmm_score", H.ptr(X), H.ptr(m["weights"]), H.ptr(m["means"]), H.ptr(m["precisions_cholesky"]),
          H.ptr(m["log_det"]), H.ptr(logdens), H.ptr(resp), H.ptr(labels), N, D, C, 1, diag, H.stream())
    return {"log_density": logdens, "labels": labels, "resp": resp, "score": float(logdens.cpu().numpy().mean())}


def gmm_sample(fit, n, u=None, eps=None, state=None, restart=None):
    """n draws from one mixture of `fit` (as in gmm_score): draw i takes the first component k with u[i] < w_0 + .. + w_k (the
    last one takes the rest) and z = mu_k + L_k eps[i] in double, rounded to fp32 once.  `u` (n,) float64 in [0, 1) (None:
    numpy.random.RandomState(0).random_sample(n)); `eps` (n,D) floats (None: ops.randn on `state`, the int32[3] state of the
    device generator).  -> (z (n,D) fp32, components (n,) int32)"""
    who = "gmm_sample"
    m, diag, _ = _gmm_mixture(who, fit, restart)
    C, D = m["means"].shape
    n = int(n)
    if not 1 <= n <= H.GMM_MAX_DRAWS:
        raise ValueError(f"{who}: n = {n} draws (1 .. {H.GMM_MAX_DRAWS} per call are on the MI355X path)")
    if u is None:
        u = torch.from_numpy(np.random.RandomState(0).random_sample(n))
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u))
    if not torch.is_tensor(u) or u.dtype != torch.float64 or u.shape != (n,):
        said = f"{tuple(u.shape)}, {u.dtype}" if torch.is_tensor(u) else type(u).__name__
        raise ValueError(f"{who}: u is {said}; float64 ({n},) values in [0, 1)")
    if not bool(((u >= 0) & (u < 1)).all()):
        raise ValueError(f"{who}: u holds values outside [0, 1)")
    if eps is None:
        if not torch.is_tensor(state) or state.dtype != torch.int32 or state.numel() != 3:
            raise ValueError(f"{who}: without eps the draws need `state`, the int32[3] state of the device generator")
        eps = randn((n, D), state)
    if not torch.is_tensor(eps) or not eps.is_floating_point() or eps.shape != (n, D):
        said = f"{tuple(eps.shape)}, {eps.dtype}" if torch.is_tensor(eps) else type(eps).__name__
        raise ValueError(f"{who}: eps is {said}; floating ({n}, {D}) standard-normal values")
    _finite(who, "eps", eps)
    dev = m["weights"].device
    if dev.type != "cuda":
        raise ValueError(f"{who}: the mixture is on {dev}; the kernels run on the MI355X (there is no host path)")
    u, eps = u.detach().to(dev).contiguous(), H.f32c(eps.detach().to(dev))
    z = torch.empty(n, D, dtype=torch.float32, device=dev)
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    _call("mmvae_gmm_sample", H.ptr(m["weights"]), H.ptr(m["means"]), H.ptr(m["cholesky"]), H.ptr(u), H.ptr(eps), H.ptr(z),
          H.ptr(comp), n, D, C, diag, H.stream())
    return z, comp


def gmm_information(fit, n_rows, restart=None):
    """BIC and AIC of one mixture of `fit` on the n_rows rows it was fitted to, on the host, as scikit-learn's
    GaussianMixture.bic / .aic: n_parameters = C D (D + 1) / 2 + C D + C - 1 (full) or 2 C D + C - 1 (diag); with score = the
    mean log-density of those rows (`fit["log_density"]` of the restart, or a single mixture's `fit["score"]`):
    bic = -2 N score + n_parameters ln N, aic = -2 N score + 2 n_parameters.  -> {"n_parameters", "bic", "aic"}"""
    who = "gmm_information"
    if not isinstance(fit, dict) or not torch.is_tensor(fit.get("means")) or "covariance_type" not in fit:
        raise ValueError(f"{who}: fit is what gmm_fit returns (means, covariance_type, log_density)")
    diag = _gmm_covariance(who, fit["covariance_type"])
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError(f"{who}: n_rows = {n_rows}")
    C, D = fit["means"].shape[-2:]
    if fit["means"].dim() == 3:
        R = fit["means"].shape[0]
        restart = fit.get("best") if restart is None else restart
        if not isinstance(restart, (int, np.integer)) or not 0 <= restart < R:
            raise ValueError(f"{who}: restart = {restart!r} (the fit holds the restarts 0 .. {R - 1})")
        rows = fit["log_density"][restart]
        if rows.shape[0] != n_rows:
            raise ValueError(f"{who}: n_rows = {n_rows}, the fit holds the log-density of {rows.shape[0]} rows")
        score = float(rows.detach().cpu().numpy().mean())
    else:
        if restart is not None:
            raise ValueError(f"{who}: restart = {restart!r} for a single mixture (None)")
        score = float(fit["score"])
    n_par = (2 * C * D if diag else C * D * (D + 1) // 2 + C * D) + C - 1
    return {"n_parameters": n_par, "bic": -2.0 * score * n_rows + n_par * math.log(n_rows),
            "aic": -2.0 * score * n_rows + 2 * n_par}


# ---- canonical correlation of feature pairs and sentence features (csrc/cca.hip): float64, forward only, no autograd ---------
def _f64_block(who, what, M):
    """a float64 (rows, cols) tensor or view whose rows are contiguous (a sub-block of a row-major matrix), or ValueError"""
    if not torch.is_tensor(M) or M.dim() != 2 or M.dtype != torch.float64 or M.stride(1) != 1 or \
            M.stride(0) < M.shape[1] or not all(1 <= n <= H.FRECHET_MAX_F for n in M.shape):
        said = f"{tuple(M.shape)}, {M.dtype}, strides {M.stride()}" if torch.is_tensor(M) else type(M).__name__
        raise ValueError(f"{who}: {what} is {said}; a float64 block (rows, cols) with contiguous rows, 1 .. "
                         f"{H.FRECHET_MAX_F} each way on the MI355X path")
    return M


def f64_gemm_ld(A, B, out, trans_b=False, scale=None):
    """out (M,N) <- (A diag(scale)) B, or (A diag(scale)) B^T for trans_b: A (M,K), B (K,N) or (N,K), `out` float64 blocks
    with contiguous rows -- slices of larger row-major matrices are read and written in place, nothing else of `out`'s
    matrix is touched.  `scale` (K,) float64 multiplies the columns of A as they are loaded (None: the plain product).  The
    fp64 MFMA tile routine of f64_gemm; M, N, K need be no multiples of its tile.  `out` must not share memory with A or
    B.  -> out"""
    who = "f64_gemm_ld"
    A, B, out = _f64_block(who, "A", A), _f64_block(who, "B", B), _f64_block(who, "out", out)
    (M, K), (N, Kb) = A.shape, (B.shape if trans_b else B.shape[::-1])
    if Kb != K or tuple(out.shape) != (M, N):
        raise ValueError(f"{who}: A {tuple(A.shape)}, B {tuple(B.shape)} (trans_b = {bool(trans_b)}), out "
                         f"{tuple(out.shape)} do not form a product")
    if scale is not None:
        if not torch.is_tensor(scale) or tuple(scale.shape) != (K,) or scale.dtype != torch.float64:
            raise ValueError(f"{who}: scale must be float64 ({K},), one factor per column of A")
        scale = scale.contiguous()
    store = out.untyped_storage().data_ptr()
    if store in (A.untyped_storage().data_ptr(), B.untyped_storage().data_ptr()):
        raise ValueError(f"{who}: out shares its memory with an operand")
    if not (A.is_cuda and B.is_cuda and out.is_cuda):
        raise ValueError(f"{who}: the blocks are on {A.device}, {B.device}, {out.device}; the kernel runs on the MI355X "
                         f"(there is no host path)")
    _call("mmvae_f64_gemm_ld", H.ptr(A), A.stride(0), H.ptr(B), B.stride(0), H.ptr(out), out.stride(0), H.ptr(scale), M, N, K,
          int(bool(trans_b)), H.stream())
    return out


def _cca_widths(who, widths, O):
    try:
        widths = [int(w) for w in widths]
    except TypeError:
        raise ValueError(f"{who}: widths = {widths!r} (the feature width of every view, in order)") from None
    if not 2 <= len(widths) <= H.CCA_MAX_VIEWS or min(widths) < 1:
        raise ValueError(f"{who}: widths = {widths} (2 .. {H.CCA_MAX_VIEWS} views of at least one feature each)")
    if sum(widths) != O:
        raise ValueError(f"{who}: widths = {widths} sum to {sum(widths)}, the moments hold O = {O} features")
    if O > H.FRECHET_MAX_F:
        raise ValueError(f"{who}: the views hold O = {O} features side by side; the eigensolver takes at most "
                         f"{H.FRECHET_MAX_F} in all (MMVAE_FRECHET_MAX_F) on the MI355X path: reduce a view's features first")
    return widths


def cca_fit(mu, sigma, widths, k, ridge=1e-12):
    """Multi-view canonical correlation analysis from the moments of the stacked views: the arithmetic of the reference's
    cca (eval/mnistsvhn_helper.py:26-78) in float64 on the device.  `mu` (O,), `sigma` (O,O): frechet_moments of rows that
    hold the views' features side by side, view i `widths[i]` wide, O = sum(widths).  The reference solves A v = lambda B v,
    B = the block diagonal of the views' covariances + ridge I, A = the off-diagonal blocks + ridge I (its quirk, kept).
    Here, with W = B^-1/2 built per view from sym_eig (B_i = Q L Q^T, W_i = Q L^-1/2 Q^T), the symmetric positive
    semi-definite N = W (sigma + 2 ridge I) W has the eigenvalues 1 + lambda and the eigenvectors u, v = W u: sym_eig(N),
    a stable descending sort (ties keep solver order), the k largest.  Every product is f64_gemm_ld on sub-blocks of
    (O,O) matrices; no block-diagonal W is multiplied out.
    -> {"correlations": (k,) float64 = value - 1, "projections": [(o_i, k) float64 per view], the columns of the stacked
        (O, k) matrix scaled to unit Euclidean norm (what scipy.linalg.eig returns; the sign of a column is the solver's),
        "means": [the slices of mu], "sweeps": {"views": [per view], "joint": of N}, "condition": [lambda_min / lambda_max
        of B_i per view], "widths", "k"}.
    2 .. 8 views, O <= 2048, 1 <= k <= min(min(widths), 64), ridge > 0.  A view whose covariance is rank-deficient is
    ill-posed at the default ridge (float64 eig(A, B) itself is): the remedy is the caller's, a ridge near 1e-3 of the
    feature variance.
    Deviations from the reference: k is required (its k=None picks k by an Otsu threshold of scikit-image, not restated);
    the covariances are float64 from the float32 features, where the reference forms them in float32 torch.mm."""
    who = "cca_fit"
    if not torch.is_tensor(sigma) or sigma.dim() != 2 or sigma.shape[0] != sigma.shape[1] or sigma.dtype != torch.float64 \
            or not torch.is_tensor(mu) or tuple(mu.shape) != (sigma.shape[0],) or mu.dtype != torch.float64:
        raise ValueError(f"{who}: mu (O,) and sigma (O,O) are the float64 moments frechet_moments returns")
    O = sigma.shape[0]
    widths = _cca_widths(who, widths, O)
    k, ridge = int(k), float(ridge)
    if not 1 <= k <= min(min(widths), H.CCA_MAX_K):
        raise ValueError(f"{who}: k = {k} (1 .. min(narrowest view = {min(widths)}, {H.CCA_MAX_K}) on the MI355X path)")
    if not (ridge > 0.0 and math.isfinite(ridge)):
        raise ValueError(f"{who}: ridge = {ridge} (a positive number: B must be positive definite)")
    if not bool(torch.isfinite(sigma).all()) or not bool(torch.isfinite(mu).all()):
        raise ValueError(f"{who}: the moments hold values that are not finite")
    if sigma.device.type != "cuda":
        raise ValueError(f"{who}: the moments are on {sigma.device}; the kernels run on the MI355X (there is no host path)")
    dev, mu = sigma.device, mu.contiguous()
    S = sigma.clone(memory_format=torch.contiguous_format)
    S.diagonal().add_(2.0 * ridge)
    offs = [0] + list(itertools.accumulate(widths))
    W = torch.zeros(O, O, dtype=torch.float64, device=dev)
    lows, highs, view_sweeps = [], [], []
    for lo, hi in zip(offs, offs[1:]):
        Bi = sigma[lo:hi, lo:hi].clone(memory_format=torch.contiguous_format)
        Bi.diagonal().add_(ridge)
        e = sym_eig(Bi)
        lam, Q = e["values"], e["vectors"].contiguous()
        lows.append(lam.min())
        highs.append(lam.max())
        view_sweeps.append(e["sweeps"])
        f64_gemm_ld(Q, Q, W[lo:hi, lo:hi], trans_b=True, scale=lam.rsqrt())
    lows, highs = torch.stack(lows).tolist(), torch.stack(highs).tolist()
    if not all(l > 0.0 for l in lows) or not bool(torch.isfinite(W).all()):
        raise ValueError(f"{who}: a view's covariance + ridge I is singular in float64 (smallest eigenvalues {lows}); "
                         f"raise `ridge`")
    T, N = torch.empty_like(W), torch.empty_like(W)
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(W[lo:hi, lo:hi], S[lo:hi, :], T[lo:hi, :])          # T = W S, a row of blocks per launch
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(T[:, lo:hi], W[lo:hi, lo:hi], N[:, lo:hi])          # N = T W, a column of blocks per launch
    N = (N + N.t()) * 0.5      # W is symmetric to rounding only; the solver wants the two halves equal
    e = sym_eig(N)
    order = torch.sort(e["values"], descending=True, stable=True).indices[:k]
    U = e["vectors"][:, order].contiguous()
    P = torch.empty(O, k, dtype=torch.float64, device=dev)
    for lo, hi in zip(offs, offs[1:]):
        f64_gemm_ld(W[lo:hi, lo:hi], U[lo:hi, :], P[lo:hi, :])
    P = P / torch.linalg.vector_norm(P, dim=0, keepdim=True)
    return {"correlations": e["values"][order] - 1.0, "projections": [P[lo:hi].contiguous() for lo, hi in zip(offs, offs[1:])],
            "means": [mu[lo:hi].contiguous() for lo, hi in zip(offs, offs[1:])],
            "sweeps": {"views": view_sweeps, "joint": e["sweeps"]}, "condition": [l / h for l, h in zip(lows, highs)],
            "widths": widths, "k": k}


def _cca_side(who, name, x, mean, proj):
    if not torch.is_tensor(x) or x.dim() != 2 or not x.is_floating_point():
        said = f"{tuple(x.shape)}, {x.dtype}" if torch.is_tensor(x) else type(x).__name__
        raise ValueError(f"{who}: {name} is {said}; floating (rows, o) features")
    o = x.shape[1]
    if not 1 <= o <= H.FRECHET_MAX_F:
        raise ValueError(f"{who}: {name} has o = {o} features (1 .. {H.FRECHET_MAX_F} are on the MI355X path)")
    for what, t, dims in ((f"mean_{name}", mean, 1), (f"proj_{name}", proj, 2)):
        if not torch.is_tensor(t) or t.dim() != dims or t.shape[0] != o or t.dtype != torch.float64:
            said = f"{tuple(t.shape)}, {t.dtype}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{who}: {what} is {said}; float64 ({o},{'' if dims == 1 else ' k'}) beside {name}")
    return x.detach(), mean.contiguous(), proj.contiguous()


def cca_score(a, b, mean_a, mean_b, proj_a, proj_b):
    """The cross-modal correlation of paired feature rows a (rows, o_a), b (rows, o_b) under a fit (cca_fit's means and
    projections, float64 (o,) and (o, k)): per row r, p = (a_r - mean_a) proj_a, q = (b_r - mean_b) proj_b and
    cos_r = p . q / (max(|p|, 1e-8) max(|q|, 1e-8)), F.cosine_similarity's clamp.  One kernel: the rows are converted and
    centred in double as they are loaded, both products run on the fp64 MFMA, the projections are never written.
    -> (cos (rows,) float64, their sum, a float64 0-d tensor added in a fixed order: two runs give the same bits)."""
    who = "cca_score"
    a, mean_a, proj_a = _cca_side(who, "a", a, mean_a, proj_a)
    b, mean_b, proj_b = _cca_side(who, "b", b, mean_b, proj_b)
    rows, k = a.shape[0], proj_a.shape[1]
    if b.shape[0] != rows or not 1 <= rows <= H.CCA_MAX_ROWS:
        raise ValueError(f"{who}: a has {rows} rows, b {b.shape[0]} (the same rows of both views, at least one)")
    if proj_b.shape[1] != k or not 1 <= k <= H.CCA_MAX_K:
        raise ValueError(f"{who}: proj_a has k = {k} columns, proj_b {proj_b.shape[1]} (the same 1 .. {H.CCA_MAX_K} on the "
                         f"MI355X path)")
    if a.device.type != "cuda":
        raise ValueError(f"{who}: a is on {a.device}; the kernel runs on the MI355X (there is no host path)")
    a, b = H.f32c(a), H.f32c(b)
    if not bool(torch.isfinite(a).all() & torch.isfinite(b).all()):      # (one read for both views)
        raise ValueError(f"{who}: the features hold values that are not finite")
    cos = torch.empty(rows, dtype=torch.float64, device=a.device)
    total = torch.empty(1, dtype=torch.float64, device=a.device)
    _call("mmvae_cca_score", H.ptr(a), H.ptr(b), H.ptr(mean_a), H.ptr(mean_b), H.ptr(proj_a), H.ptr(proj_b), H.ptr(cos),
          H.ptr(total), rows, a.shape[1], b.shape[1], k, H.stream())
    return cos, total[0]


def sentence_features(ids, emb, weights, eos=2, pc=None):
    """Frequency-weighted sentence embeddings, the reference's apply_weights and apply_pc (eval/mnistsvhn_helper.py:165-177):
    ids (B, T) integer tokens, emb (V, E) the embedding table, weights (V,) the tokens' weights (coherence.sif_weights).
    Per sentence L = index of the first `eos` + 1 (T without one), f = (sum_{t < L} weights[id_t] emb[id_t]) / L in double
    in token order; with `pc` (E,) float64, a unit vector, f <- f - pc (pc . f), the common component removed.  One wave per
    sentence, one rounding to fp32.  -> (B, E) fp32.  1 <= E <= 1024, 1 <= T <= 512; every id must lie in [0, V)."""
    who = "sentence_features"
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
        raise ValueError(f"{who}: ids are integer (B, T) tokens")
    if not torch.is_tensor(emb) or emb.dim() != 2 or not emb.is_floating_point():
        raise ValueError(f"{who}: emb is the floating (V, E) embedding table")
    (B, T), (V, E) = ids.shape, emb.shape
    if not 1 <= E <= H.SENTENCE_MAX_E or not 1 <= T <= H.SENTENCE_MAX_T or B < 1 or V < 1:
        raise ValueError(f"{who}: B = {B} sentences of T = {T} tokens, V = {V} embeddings of E = {E} (1 <= T <= "
                         f"{H.SENTENCE_MAX_T}, 1 <= E <= {H.SENTENCE_MAX_E} are on the MI355X path)")
    if not torch.is_tensor(weights) or tuple(weights.shape) != (V,) or not weights.is_floating_point():
        raise ValueError(f"{who}: weights are floating ({V},), one per embedding")
    if pc is not None and (not torch.is_tensor(pc) or tuple(pc.shape) != (E,) or pc.dtype != torch.float64):
        raise ValueError(f"{who}: pc is a float64 ({E},) unit vector, or None")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"{who}: ids in [{lo}, {hi}] outside the table's [0, {V})")
    if emb.device.type != "cuda":
        raise ValueError(f"{who}: emb is on {emb.device}; the kernel runs on the MI355X (there is no host path)")
    dev = emb.device
    ids = ids.detach().to(device=dev, dtype=torch.int32).contiguous()
    emb, weights = H.f32c(emb.detach()), H.f32c(weights.detach().to(dev))
    pc = None if pc is None else pc.detach().to(dev).contiguous()
    out = torch.empty(B, E, dtype=torch.float32, device=dev)
    _call("mmvae_sentence_features", H.ptr(ids), H.ptr(emb), H.ptr(weights), H.ptr(pc), H.ptr(out), B, T, E, V, int(eos),
          H.stream())
    return out


# ---- image reconstruction quality (csrc/image_quality.hip): PSNR, SSIM, MS-SSIM; float64, forward only -------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003, five scales


def image_quality_window(win=11, sigma=1.5):
    """the 1-D window weights in double, summing to 1 (their outer product is the 2-D window): g[i] ~ exp(-(i - (win - 1) / 2)^2
    / (2 sigma^2)), or 1 / win each for sigma None"""
    if sigma is None:
        return np.full(win, 1.0 / win)
    g = np.exp(-((np.arange(win, dtype=np.float64) - (win - 1) / 2.0) ** 2) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def image_quality(x, y, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1, weights=None):
    """How close the images y are to the images x, pair by pair: x, y floating (N, C, H, W), read as fp32, everything after
    the load in float64, one launch, one workgroup per pair (csrc/image_quality.hip; mmvae_hip.h has the arithmetic).
      mse, mae   means of (x - y)^2 and |x - y| over C H W;  psnr = 10 log10(data_range^2 / mse), +inf for mse = 0;
      ssim       Wang et al. 2004: the mean over the C planes of the mean over the (H - win + 1)(W - win + 1) valid window
                 positions (no padding) of l cs, l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), cs = (2 s_xy + C2) /
                 (s_x^2 + s_y^2 + C2), C1 = (k1 data_range)^2, C2 = (k2 data_range)^2, moments under the window: Gaussian
                 of `sigma` (the paper's: win 11, sigma 1.5), or uniform for sigma None; `sample_covariance` scales the
                 (co)variances by win^2 / (win^2 - 1) (scikit-image's default call: win 7, sigma None, sample_covariance True);
      ms_ssim    `scales` = S levels, level s + 1 the 2 x 2 average pooling of level s (needs even sides; every level sides >=
                 win): prod_{s < S} max(cs_s, 0)^w_s max(l_S, 0)^w_S of the image's per-level means (over positions, then
                 channels), clamped at 0 before the powers; S = 1: max(ssim, 0).  `weights` (S,) default to the first S of
                 (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) divided by their sum -- for S < 5 that is NOT the five-scale
                 standard, whose images must have sides >= 16 win;
      levels     (N, S): cs_1 .. cs_{S-1}, l_S.
    -> {"mse", "mae", "psnr", "ssim", "ms_ssim": (N,) float64, "levels": (N, S) float64} on the device.  No map and no pooled
    plane is written, no atomics, every sum in a fixed order: a row's bits do not depend on the other rows of the call.
    win odd in 3 .. 11, win <= H, W <= 64, 1 <= C <= 4, 1 <= S <= 4, finite inputs."""
    who = "image_quality"
    for what, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point():
            said = f"{tuple(t.shape)}, {t.dtype}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{who}: {what} is {said}; floating (N, C, H, W) images")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"{who}: x is {tuple(x.shape)} on {x.device}, y {tuple(y.shape)} on {y.device} (pairs of images: the "
                         f"same shape and device)")
    N, C, Hh, W = x.shape
    plan = image_quality_plan((N, C, Hh, W), win, sigma, data_range, k1, k2, sample_covariance, scales, weights)
    if x.device.type != "cuda":
        raise ValueError(f"{who}: x is on {x.device}; the kernel runs on the MI355X (there is no host path)")
    x, y = H.f32c(x.detach()), H.f32c(y.detach())
    _finite(who, "x", x)
    _finite(who, "y", y)
    win, S = plan["win"], plan["scales"]
    out = torch.empty(N, 5 + S, dtype=torch.float64, device=x.device)
    _call("mmvae_image_quality", H.ptr(x), H.ptr(y), H.ptr(out), N, C, Hh, W, win, (ctypes.c_double * win)(*plan["window"]),
          plan["data_range"], plan["c1"], plan["c2"], plan["cov_scale"], S, (ctypes.c_double * S)(*plan["weights"]), H.stream())
    return {"mse": out[:, 0], "mae": out[:, 1], "psnr": out[:, 2], "ssim": out[:, 3], "ms_ssim": out[:, 4],
            "levels": out[:, 5:]}


def image_quality_plan(shape, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1,
                       weights=None):
    """image_quality's checks of its arguments against the images' shape (N, C, H, W), before any device call: ValueError, or
    -> {"win", "scales", "window": win doubles, "weights": S doubles, "data_range", "c1", "c2", "cov_scale"}"""
    who = "image_quality"
    N, C, Hh, W = (int(v) for v in shape)
    win, S = int(win), int(scales)
    if not H.IQ_MIN_WIN <= win <= H.IQ_MAX_WIN or win % 2 == 0:
        raise ValueError(f"{who}: win = {win} (odd, {H.IQ_MIN_WIN} .. {H.IQ_MAX_WIN} are on the MI355X path)")
    if not (win <= Hh <= H.IQ_MAX_SIDE and win <= W <= H.IQ_MAX_SIDE):
        raise ValueError(f"{who}: planes of {Hh} x {W} for win = {win} (sides of win .. {H.IQ_MAX_SIDE} are on the MI355X path)")
    if not 1 <= C <= H.IQ_MAX_CHANNELS or not 1 <= N <= H.IQ_MAX_ROWS:
        raise ValueError(f"{who}: {N} images of {C} channels (at least one image, 1 .. {H.IQ_MAX_CHANNELS} channels are on the "
                         f"MI355X path)")
    if not 1 <= S <= H.IQ_MAX_SCALES:
        raise ValueError(f"{who}: scales = {S} (1 .. {H.IQ_MAX_SCALES} are on the MI355X path)")
    h, w = Hh, W
    for level in range(2, S + 1):
        if h % 2 or w % 2:
            raise ValueError(f"{who}: level {level - 1} is {h} x {w}; pooling it into level {level} needs even sides")
        h, w = h // 2, w // 2
        if h < win or w < win:
            raise ValueError(f"{who}: level {level} is {h} x {w}, smaller than win = {win} ({Hh} x {W} images allow scales <= "
                             f"{level - 1})")
    if sigma is not None and not (math.isfinite(float(sigma)) and float(sigma) > 0.0):
        raise ValueError(f"{who}: sigma = {sigma} (a positive width, or None for the uniform window)")
    L, k1, k2 = float(data_range), float(k1), float(k2)
    if not (math.isfinite(L) and L > 0.0 and math.isfinite(k1) and k1 > 0.0 and math.isfinite(k2) and k2 > 0.0):
        raise ValueError(f"{who}: data_range = {data_range}, k1 = {k1}, k2 = {k2} (positive and finite)")
    if weights is None:
        msw = np.asarray(MS_SSIM_WEIGHTS[:S], dtype=np.float64)
        msw = msw / msw.sum()
    else:
        msw = np.asarray(weights.detach().cpu().double().numpy() if torch.is_tensor(weights) else weights,
                         dtype=np.float64).reshape(-1)
        if msw.shape[0] != S or not np.all(np.isfinite(msw)) or np.any(msw < 0.0):
            raise ValueError(f"{who}: weights holds {msw.shape[0]} values for scales = {S} (one finite exponent >= 0 per level)")
    return {"win": win, "scales": S, "window": image_quality_window(win, sigma).tolist(), "weights": msw.tolist(),
            "data_range": L, "c1": (k1 * L) ** 2, "c2": (k2 * L) ** 2,
            "cov_scale": win * win / (win * win - 1.0) if sample_covariance else 1.0}


# ---- text generation quality (csrc/text_quality.hip): edit distance, BLEU and ROUGE-L counts, NLL; forward only -----------------
def text_quality_plan(Th, Tr, V, eos=None, trim=None, sep=None, max_order=4):
    """text_quality's checks of its arguments against the sequences' steps Th (hypothesis), Tr (reference) and the
    vocabulary V, before any device call: ValueError, or -> {"eos", "trim", "sep": ids, -1 for None; "max_order"}"""
    who = "text_quality"
    Th, Tr, V, K = int(Th), int(Tr), int(V), int(max_order)
    if not (1 <= Th <= H.TQ_MAX_STEPS and 1 <= Tr <= H.TQ_MAX_STEPS):
        raise ValueError(f"{who}: hypotheses of {Th} steps, references of {Tr} (1 .. {H.TQ_MAX_STEPS} steps are on the MI355X "
                         f"path)")
    if not 2 <= V <= H.TQ_MAX_VOCAB:
        raise ValueError(f"{who}: V = {V} (2 .. {H.TQ_MAX_VOCAB} symbols are on the MI355X path)")
    if not 1 <= K <= H.TQ_MAX_ORDER:
        raise ValueError(f"{who}: max_order = {K} (n-gram orders 1 .. {H.TQ_MAX_ORDER})")
    ids = {}
    for what, v in (("eos", eos), ("trim", trim), ("sep", sep)):
        if v is not None and (isinstance(v, bool) or int(v) != v or not 0 <= int(v) < V):
            raise ValueError(f"{who}: {what} = {v!r} (a token id in [0, {V}), or None)")
        ids[what] = -1 if v is None else int(v)
    if ids["sep"] >= 0 and ids["sep"] == ids["eos"]:
        raise ValueError(f"{who}: sep = eos = {ids['sep']} (the separator must differ from the end marker)")
    return dict(ids, max_order=K)


def _tq_ids(who, what, t, shape, V):
    """contiguous int32 ids of `shape` (a None entry: any size >= 1), every id in [0, V) (V None: unchecked), or ValueError"""
    if not torch.is_tensor(t) or t.dim() != len(shape) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        said = f"{tuple(t.shape)}, {t.dtype}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{who}: {what} is {said}; integers of shape {shape}".replace("None", "T"))
    if any(s is not None and d != s for d, s in zip(t.shape, shape)):
        raise ValueError(f"{who}: {what} is {tuple(t.shape)}, not {shape}".replace("None", "T"))
    t = t.detach()
    if V is not None and t.numel() and not (0 <= int(t.min()) and int(t.max()) < V):
        raise ValueError(f"{who}: {what} holds ids from {int(t.min())} to {int(t.max())} (token ids lie in [0, {V}))")
    return t.to(torch.int32).contiguous()


def text_quality(hyp, ref_ids, ref_lengths, hyp_lengths=None, eos=None, trim=None, sep=None, max_order=4):
    """How close the token sequences `hyp` are to the references, pair by pair, in one launch, one wave per pair
    (csrc/text_quality.hip; mmvae_hip.h has the arithmetic).  hyp: floating (N, Th, V) logits, read as fp32 -- the hypothesis
    is their argmax, the first maximum of every step -- or integer (N, Th) ids.  ref_ids integer (N, Tr), ref_lengths integer
    (N,), hyp_lengths integer (N,) or None (Th each); lengths are clamped into [0, T].  eos: a sequence ends before its first
    eos; trim: trailing tokens equal to trim are then dropped; both sides alike, giving h (Lh tokens) and r (Lr).
      token   hyp_len Lh, ref_len Lr, same = #{t < min(Lh, Lr): h_t == r_t}, edit = Levenshtein distance, lcs = longest common
              subsequence, match (N, 4) / total (N, 4): for n = 1 .. max_order the clipped n-gram matches sum_g min(count_h(g),
              count_r(g)) and max(Lh - n + 1, 0); columns n > max_order are 0.
      word    with sep: the same (without `same`) over the words, the maximal runs of tokens != sep; None without.
      pred    (N, Th) the argmax;  nll (N,) float64 = sum_{t < S} (logsumexp(x_t) - x_t[ref_t]), S = min(ref length, Th) =
              nll_steps (N,): before eos / trim, the decoder's objective.  All three None for an ids hypothesis.
    -> {"token": {...}, "word": {...} or None, "pred", "nll", "nll_steps", "max_order"}, int32 tensors on the device.  No
    atomics; a pair's outputs do not depend on the other pairs.  1 <= Th, Tr <= 256, 2 <= V <= 256 (ids form: ids < 256),
    ids in [0, V), sep != eos.  The logits are expected finite and are not scanned (torch's isfinite().all() is five launches over
    the whole tensor): a step that holds a NaN or +inf shows as a NaN in the pair's nll."""
    who = "text_quality"
    if not torch.is_tensor(hyp) or not ((hyp.is_floating_point() and hyp.dim() == 3) or
                                        (not hyp.is_floating_point() and hyp.dim() == 2)):
        said = f"{tuple(hyp.shape)}, {hyp.dtype}" if torch.is_tensor(hyp) else type(hyp).__name__
        raise ValueError(f"{who}: hyp is {said}; floating (N, Th, V) logits or integer (N, Th) ids")
    logits = hyp.is_floating_point()
    N, Th = hyp.shape[:2]
    V = hyp.shape[2] if logits else H.TQ_MAX_VOCAB
    if not torch.is_tensor(ref_ids) or ref_ids.dim() != 2:
        said = f"{tuple(ref_ids.shape)}, {ref_ids.dtype}" if torch.is_tensor(ref_ids) else type(ref_ids).__name__
        raise ValueError(f"{who}: ref_ids is {said}; integers of shape (N, Tr)")
    Tr = ref_ids.shape[1]
    if not 1 <= N <= H.TQ_MAX_ROWS:
        raise ValueError(f"{who}: {N} pairs (1 .. {H.TQ_MAX_ROWS} a call: one workgroup per pair in one launch)")
    plan = text_quality_plan(Th, Tr, V, eos, trim, sep, max_order)
    ref_ids = _tq_ids(who, "ref_ids", ref_ids, (N, None), V)
    ref_lengths = _tq_ids(who, "ref_lengths", ref_lengths, (N,), None)
    if hyp_lengths is not None:
        hyp_lengths = _tq_ids(who, "hyp_lengths", hyp_lengths, (N,), None)
    hyp = H.f32c(hyp.detach()) if logits else _tq_ids(who, "hyp", hyp, (N, Th), V)
    dev = hyp.device
    if any(t is not None and t.device != dev for t in (ref_ids, ref_lengths, hyp_lengths)):
        raise ValueError(f"{who}: hyp is on {dev}, the references or lengths elsewhere (one device)")
    if dev.type != "cuda":
        raise ValueError(f"{who}: hyp is on {dev}; the kernel runs on the MI355X (there is no host path)")
    K = plan["max_order"]
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    tok, word = i32(N, 13), (i32(N, 12) if plan["sep"] >= 0 else None)
    pred, nll, steps = (i32(N, Th), torch.empty(N, dtype=torch.float64, device=dev), i32(N)) if logits else (None,) * 3
    _call("mmvae_text_quality", H.ptr(hyp) if logits else None, None if logits else H.ptr(hyp), H.ptr(ref_ids),
          H.ptr(ref_lengths), H.ptr(hyp_lengths), H.ptr(pred), H.ptr(tok), H.ptr(word), H.ptr(nll), H.ptr(steps), N, Th, Tr, V,
          plan["eos"], plan["trim"], plan["sep"], K, H.stream())
    level = lambda o, same: dict(
        {"hyp_len": o[:, 0], "ref_len": o[:, 1], "edit": o[:, 2 + same], "lcs": o[:, 3 + same],
         "match": o[:, 4 + same:8 + same], "total": o[:, 8 + same:12 + same]}, **({"same": o[:, 2]} if same else {}))
    return {"token": level(tok, 1), "word": None if word is None else level(word, 0), "pred": pred, "nll": nll,
            "nll_steps": steps, "max_order": K}


def _tq_level_summary(parts, K, token):
    """the summary of one level from the per-pair integer counts of `parts` (dicts of (n,) / (n, 4) integer tensors)"""
    cat = lambda name: np.concatenate([p[name].detach().cpu().numpy().astype(np.int64) for p in parts])
    hl, rl, edit, lcs, match, total = (cat(k) for k in ("hyp_len", "ref_len", "edit", "lcs", "match", "total"))
    n = len(hl)
    Hs, Rs = int(hl.sum()), int(rl.sum())
    ms, ts = [int(v) for v in match[:, :K].sum(0)], [int(v) for v in total[:, :K].sum(0)]
    bp = lambda h, r: math.exp(1.0 - r / h) if h < r else 1.0
    if Hs == 0 or any(m == 0 for m in ms):
        bleu = 0.0
    else:
        bleu = bp(Hs, Rs) * math.exp(sum(math.log(m / t) for m, t in zip(ms, ts)) / K)
    sent, rouge = [], []
    for i in range(n):
        h, r, l = int(hl[i]), int(rl[i]), int(lcs[i])
        if h == 0 or match[i, 0] == 0:
            sent.append(0.0)
        else:
            logs = [math.log(int(match[i, 0]) / int(total[i, 0]))]
            logs += [math.log((int(match[i, k]) + 1) / (int(total[i, k]) + 1)) for k in range(1, K)]
            sent.append(bp(h, r) * math.exp(sum(logs) / K))
        P, R = (l / h if h else 0.0), (l / r if r else 0.0)
        rouge.append(2.0 * P * R / (P + R) if P + R > 0.0 else 0.0)
    E = int(edit.sum())
    out = {"n": n, "error_rate": E / Rs if Rs else (0.0 if E == 0 else float("inf")),
           "exact": float(np.count_nonzero(edit == 0)) / n, "bleu": bleu,
           "precisions": [m / t if t else 0.0 for m, t in zip(ms, ts)], "sentence_bleu": math.fsum(sent) / n,
           "rouge_l": math.fsum(rouge) / n}
    if token:
        out["accuracy"] = int(cat("same").sum()) / Rs if Rs else 0.0
    return out


def text_quality_summary(parts):
    """The corpus figures of one or several text_quality results (a dict, or a list of them with one max_order), on the host,
    from the INTEGER sums of the per-pair counts.  -> {"token": S, "word": S or None}, S per level:
      n               pairs;
      error_rate      sum edit / sum ref_len: the character / word error rate (CER / WER) where a token is a character
                      (0 / 0 = 0, x / 0 = inf);
      exact           mean(edit == 0);
      accuracy        sum same / sum ref_len (token level only);
      bleu            corpus BLEU (Papineni et al. 2002): brevity penalty times the geometric mean over the orders 1 .. K of
                      sum match_n / sum total_n; brevity penalty exp(1 - sum ref_len / sum hyp_len) when sum hyp_len <
                      sum ref_len; 0 when a sum match_n or sum hyp_len is 0;
      precisions      [sum match_n / sum total_n for n = 1 .. K] (0 for an empty total);
      sentence_bleu   mean over the pairs of the pair's BLEU with Lin & Och's (2004) add-one smoothing of the orders n >= 2,
                      (match_n + 1) / (total_n + 1), order 1 unsmoothed (no unigram match: 0), the pair's own brevity penalty,
                      0 for an empty hypothesis;
      rouge_l         mean over the pairs of F1 = 2 P R / (P + R), P = lcs / hyp_len, R = lcs / ref_len (a zero denominator: 0);
      nll, perplexity, bits_per_token   (token level; None for ids hypotheses) sum nll / sum nll_steps, its exp, and it
                      divided by ln 2; nan when no step was scored."""
    parts = [parts] if isinstance(parts, dict) else list(parts)
    if not parts:
        raise ValueError("text_quality_summary: no parts")
    K = {int(p["max_order"]) for p in parts}
    if len(K) != 1 or len({p["word"] is None for p in parts}) != 1 or len({p["nll"] is None for p in parts}) != 1:
        raise ValueError("text_quality_summary: the parts were scored with different max_order, sep or hypothesis forms")
    K = K.pop()
    token = _tq_level_summary([p["token"] for p in parts], K, True)
    word = None if parts[0]["word"] is None else _tq_level_summary([p["word"] for p in parts], K, False)
    if parts[0]["nll"] is None:
        token.update(nll=None, perplexity=None, bits_per_token=None)
    else:
        steps = sum(int(p["nll_steps"].sum()) for p in parts)
        total = math.fsum(v for p in parts for v in p["nll"].detach().cpu().tolist())
        mean = total / steps if steps else float("nan")
        token.update(nll=mean, perplexity=math.exp(mean), bits_per_token=mean / math.log(2.0))
    return {"token": token, "word": word}


# ---- aggregate posterior, ELBO decomposition and mutual information gap (csrc/aggpost.hip): float64, forward only -----------
def _aggpost_rows(who, what, X, like=None):
    """contiguous fp32 (N, D) or ValueError: shape, dtype, the limits, the shape and device of `like`, finite values"""
    if not torch.is_tensor(X) or X.dim() != 2 or not X.is_floating_point():
        said = f"{tuple(X.shape)}, {X.dtype}" if torch.is_tensor(X) else type(X).__name__
        raise ValueError(f"{who}: {what} is {said}; floating (N, D)")
    N, D = X.shape
    if not 1 <= N <= H.AGGPOST_MAX_ROWS or not 1 <= D <= H.AGGPOST_MAX_DIM:
        raise ValueError(f"{who}: {what} is {N} x {D} (1 .. {H.AGGPOST_MAX_ROWS} rows of 1 .. {H.AGGPOST_MAX_DIM} dimensions "
                         f"are on the MI355X path)")
    if like is not None and (X.shape != like.shape or X.device != like.device):
        raise ValueError(f"{who}: {what} is {tuple(X.shape)} on {X.device}, z {tuple(like.shape)} on {like.device}")
    if not X.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    X = X.detach()
    X = X.float() if X.dtype != torch.float32 else X
    if not bool(torch.isfinite(X).all()):
        raise ValueError(f"{who}: {what} holds values that are not finite")
    return X


def _aggpost_labels(who, labels, N, device):
    """contiguous int32 (K, N) on `device` or ValueError: an integer (K, N) tensor, 1 <= K <= the limit, labels >= 0"""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.is_floating_point() or labels.is_complex() \
            or labels.dtype == torch.bool:
        said = f"{tuple(labels.shape)}, {labels.dtype}" if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"{who}: labels is {said}; an integer (K, N) tensor, one row per generative factor")
    K = labels.shape[0]
    if not 1 <= K <= H.AGGPOST_MAX_FACTORS or labels.shape[1] != N:
        raise ValueError(f"{who}: labels is {tuple(labels.shape)}; (K, {N}) with 1 <= K <= {H.AGGPOST_MAX_FACTORS} factors")
    if labels.device != device:
        raise ValueError(f"{who}: labels is on {labels.device}, z on {device}")
    if not labels.is_contiguous():
        raise ValueError(f"{who}: labels is not contiguous")
    labels = labels.detach()
    if int(labels.min()) < 0 or int(labels.max()) > 2 ** 31 - 1:
        raise ValueError(f"{who}: labels holds values outside [0, 2^31) (classes are numbered from 0)")
    return labels.to(torch.int32)


def aggregate_posterior(z, loc, scale, laplace=False, labels=None, chunks=0):
    """The aggregate posterior q(z) = (1/N) sum_m q(z | x_m) at every sample: z, loc, scale (N,D), row n of z a draw from
    posterior n = Normal | Laplace (`laplace`) (loc_n, scale_n); labels (K,N) integers >= 0, one row per generative factor,
    or None.  With l[n,m,d] = log q(z_nd | x_m) in double from the fp32 inputs:
      joint (N,)              log q(z_n)  = logsumexp_m sum_d l[n,m,d] - log N
      marginal (N,D)          log q(z_nd) = logsumexp_m l[n,m,d] - log N
      conditional (K,N,D)     logsumexp over the m that share factor k's value with n of l[n,m,d] - log(class size); None
                              without labels
      self (N,)               sum_d l[n,n,d] = log q(z_n | x_n)       (torch float64 on the device)
    float64; the N x N x D terms are never written.  `chunks`: how many workgroups share a row's posterior rows (0: the
    default plan); two plans regroup fp64 sums (agreement to rounding, not bit for bit), two runs with one plan give the
    same bits.  A z that lies so far from its own posterior that exp overflows raises FloatingPointError."""
    who = "aggregate_posterior"
    chunks = _chunks(who, chunks, "chunks")
    z = _aggpost_rows(who, "z", z)
    loc, scale = _aggpost_rows(who, "loc", loc, z), _aggpost_rows(who, "scale", scale, z)
    if not bool((scale > 0).all()):
        raise ValueError(f"{who}: scale holds values that are not positive")
    N, D = z.shape
    lab = None if labels is None else _aggpost_labels(who, labels, N, z.device)
    K, laplace = 0 if lab is None else lab.shape[0], bool(laplace)
    if z.device.type != "cuda":
        raise ValueError(f"{who}: z is on {z.device}; the kernel runs on the MI355X (there is no host path)")
    ws = torch.empty(H.lib().mmvae_aggpost_ws_doubles(N, D, K, chunks), dtype=torch.float64, device=z.device)
    joint = torch.empty(N, dtype=torch.float64, device=z.device)
    marginal = torch.empty(N, D, dtype=torch.float64, device=z.device)
    cond = None if lab is None else torch.empty(K, N, D, dtype=torch.float64, device=z.device)
    _call("mmvae_aggpost_lse", H.ptr(z), H.ptr(loc), H.ptr(scale), int(laplace), H.ptr(lab), H.ptr(ws), H.ptr(joint),
          H.ptr(marginal), H.ptr(cond), N, D, K, chunks, H.stream())
    s = scale.double()
    t = (z.double() - loc.double()) / s
    own = (-t.abs() - torch.log(2.0 * s)) if laplace else (-0.5 * t * t - torch.log(s) - 0.5 * math.log(2.0 * math.pi))
    if not bool(torch.isfinite(joint).all()) or not bool(torch.isfinite(marginal).all()):
        raise FloatingPointError(f"{who}: a row of z lies so far from its own posterior that exp(l - l[n,n]) overflows "
                                 f"(z must be a draw from the posterior of its row)")
    return {"joint": joint, "marginal": marginal, "conditional": cond, "self": own.sum(1)}


_AGG_KEYS = ("joint", "marginal", "conditional", "self")


def _aggpost_result(who, agg):
    """the (joint, marginal, conditional, self) of an aggregate_posterior result or ValueError"""
    if not isinstance(agg, dict) or any(k not in agg for k in _AGG_KEYS):
        raise ValueError(f"{who}: agg must be the dict aggregate_posterior returns ({', '.join(_AGG_KEYS)})")
    joint, marginal, cond, own = (agg[k] for k in _AGG_KEYS)
    for what, t, dims in (("joint", joint, 1), ("marginal", marginal, 2), ("self", own, 1)):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != dims:
            raise ValueError(f"{who}: agg[{what!r}] must be a float64 tensor of {dims} dimension(s)")
    N, D = marginal.shape
    if joint.shape != (N,) or own.shape != (N,) or N < 1 or D < 1:
        raise ValueError(f"{who}: agg holds joint {tuple(joint.shape)}, self {tuple(own.shape)}, marginal {(N, D)}")
    if cond is not None and (not torch.is_tensor(cond) or cond.dtype != torch.float64 or cond.dim() != 3
                             or cond.shape[1:] != (N, D)):
        raise ValueError(f"{who}: agg['conditional'] must be None or float64 (K, {N}, {D})")
    return joint, marginal, cond, own


def elbo_decomposition(agg, lpz):
    """The decomposition of the ELBO's KL term (Chen et al. 2018) from an aggregate_posterior result and lpz (N,) = sum_d
    log p(z_nd) under the prior:
      mi   = mean_n(log q(z_n | x_n) - log q(z_n))         index-code mutual information
      tc   = mean_n(log q(z_n) - sum_d log q(z_nd))        total correlation
      dwkl = mean_n(sum_d log q(z_nd) - log p(z_n))        dimension-wise KL
      kl   = mean_n(log q(z_n | x_n) - log p(z_n))         = mi + tc + dwkl
    -> 0-d float64 tensors on the device."""
    who = "elbo_decomposition"
    joint, marginal, _, own = _aggpost_result(who, agg)
    if not torch.is_tensor(lpz) or lpz.shape != joint.shape or not lpz.is_floating_point():
        said = f"{tuple(lpz.shape)}, {lpz.dtype}" if torch.is_tensor(lpz) else type(lpz).__name__
        raise ValueError(f"{who}: lpz is {said}; floating ({joint.shape[0]},), the prior's log-density of every row of z")
    if lpz.device != joint.device:
        raise ValueError(f"{who}: lpz is on {lpz.device}, agg on {joint.device}")
    lpz = lpz.detach().double()
    if not bool(torch.isfinite(lpz).all()):
        raise ValueError(f"{who}: lpz holds values that are not finite")
    sum_marginal = marginal.sum(1)
    return {"mi": (own - joint).mean(), "tc": (joint - sum_marginal).mean(), "dwkl": (sum_marginal - lpz).mean(),
            "kl": (own - lpz).mean()}


def mutual_information_gap(agg, labels):
    """The mutual information gap (Chen et al. 2018) from an aggregate_posterior result that was given `labels` (K,N):
      h_z (D,)         H(z_d) = -mean_n log q(z_nd)
      mi (K,D)         I(z_d; v_k) = H(z_d) - H(z_d | v_k), H(z_d | v_k) = -mean_n conditional[k,n,d] (the mean over all n
                       weights every class by its frequency)
      h_v (K,)         H(v_k) from the class counts
      per_factor (K,)  (largest - second largest of mi[k,:]) / H(v_k);  mig = their mean
    float64 on the device.  D >= 2, and every factor must take at least two values (H(v_k) > 0)."""
    who = "mutual_information_gap"
    _, marginal, cond, _ = _aggpost_result(who, agg)
    if cond is None:
        raise ValueError(f"{who}: agg holds no conditional (aggregate_posterior was called without labels)")
    N, D = marginal.shape
    lab = _aggpost_labels(who, labels, N, marginal.device)
    if lab.shape[0] != cond.shape[0]:
        raise ValueError(f"{who}: labels has {lab.shape[0]} factors, agg['conditional'] {cond.shape[0]}")
    if D < 2:
        raise ValueError(f"{who}: D = {D} latent dimension (the gap is between the two most informative dimensions)")
    h_v = []
    for k in range(lab.shape[0]):
        p = torch.bincount(lab[k].long()).double() / N
        p = p[p > 0]
        if p.numel() < 2:
            raise ValueError(f"{who}: factor {k} of labels takes a single value (H(v) = 0: the gap is not defined)")
        h_v.append(-(p * p.log()).sum())
    h_v = torch.stack(h_v)
    h_z = -marginal.mean(0)
    mi = h_z.unsqueeze(0) + cond.mean(1)
    top = mi.topk(2, dim=1).values
    per = (top[:, 0] - top[:, 1]) / h_v
    return {"mig": per.mean(), "per_factor": per, "mi": mi, "h_z": h_z, "h_v": h_v}


def digit_hidden(state, kinds, images):
    """-> (nets,N,50) fp32: relu(fc1) of the digit classifiers, dropout off (the features of DigitClassifier.features)"""
    kinds, ktab, xtab, _, N = _digit_args(state, kinds, images)
    hidden = torch.empty(len(kinds), N, 50, device=state.device)
    if N > 0:
        _call("mmvae_digit_hidden", H.ptr(state), ktab, xtab, H.ptr(hidden), len(kinds), state.shape[2], N, H.stream())
    return hidden


# ---- cross-modal retrieval of latents (csrc/retrieval.hip): float64 distances, exact ranks, forward only ---------------------
def _retrieval_sets(who, what, X, like=None):
    """contiguous fp32 (S, N, D) or ValueError: shape, dtype, the limits, the shape and device of `like`, finite values"""
    if not torch.is_tensor(X) or X.dim() != 3 or not X.is_floating_point():
        said = f"{tuple(X.shape)}, {X.dtype}" if torch.is_tensor(X) else type(X).__name__
        raise ValueError(f"{who}: {what} is {said}; floating (S, N, D), one (N, D) set of rows per modality")
    S, N, D = X.shape
    if not 2 <= S <= H.RETRIEVAL_MAX_SETS or not 1 <= N <= H.RETRIEVAL_MAX_ROWS or not 1 <= D <= H.RETRIEVAL_MAX_DIM:
        raise ValueError(f"{who}: {what} is {S} sets of {N} x {D} (2 .. {H.RETRIEVAL_MAX_SETS} sets of 1 .. "
                         f"{H.RETRIEVAL_MAX_ROWS} rows of 1 .. {H.RETRIEVAL_MAX_DIM} dimensions are on the MI355X path)")
    if like is not None and (X.shape != like.shape or X.device != like.device):
        raise ValueError(f"{who}: {what} is {tuple(X.shape)} on {X.device}, loc {tuple(like.shape)} on {like.device}")
    X = X.detach()
    X = (X.float() if X.dtype != torch.float32 else X).contiguous()
    _finite(who, what, X)
    return X


def _retrieval_ints(who, what, t, form):
    """an integer tensor on the host from a tensor, an array or nested lists, or ValueError naming the `form` wanted"""
    if not torch.is_tensor(t):
        try:
            t = torch.from_numpy(np.ascontiguousarray(t))
        except TypeError:
            raise ValueError(f"{who}: {what} is {type(t).__name__}; {form}") from None
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{who}: {what} is {tuple(t.shape)}, {t.dtype}; {form}")
    return t.detach().cpu()


def retrieval_pairs(S):
    """every ordered pair (query set, gallery set) of S different sets, in lexicographic order: S (S - 1) pairs"""
    return [(a, b) for a in range(int(S)) for b in range(int(S)) if a != b]


def retrieval_ranks(loc, scale=None, pairs=None, match=None, metric="l2", keep=0, chunks=0):
    """Retrieval of one set of rows from another, for P ordered pairs of the S sets of `loc` (S, N, D) (the latent means of S
    modalities, say; `scale` (S, N, D) their standard deviations): per pair (query set, gallery set) and query row i, where
    does the gallery row match[i] -- the row of the same sample -- rank among all N gallery rows by distance to the query?
      metric "l2"      sum (mq - mg)^2                    "cosine"  1 - mq . mg / (|mq| |mg|), 1 when either norm is 0
             "w2"      sum (mq - mg)^2 + (sq - sg)^2      "skl"     KL(q || g) + KL(g || q) of diagonal Gaussians
      (w2, skl: `scale` is needed, > 0), in double from the fp32 values by direct differences; a pair's distance is a function
      of its two rows alone, so the comparisons are exact with respect to these distances.
    `pairs`: integer (P, 2) (query set, gallery set), the two different; None: retrieval_pairs(S).  `match`: integer (N,), -1
    for a row without a partner; None: the identity.  `keep` <= 16 nearest gallery rows are returned per query.
    -> {"d_match" (P, N) float64 (NaN without a partner), "less", "equal" (P, N) int32: the gallery rows other than the
        partner that are nearer / exactly as near (-1 without a partner), "nn_d" (P, N, keep) float64 ascending, "nn_idx" (P, N,
        keep) int32, ordered by (distance, index), padded with (+inf, -1) when N < keep, "pairs": the list of pairs}.
    The N x N distances are never written.  `chunks`: how many workgroups share a row's gallery rows (0: the default plan);
    the result does not depend on it, nor on what other pairs the call holds, bit for bit."""
    who = "retrieval_ranks"
    if metric not in H.RETRIEVAL_METRICS:
        raise ValueError(f"{who}: metric = {metric!r} ({', '.join(H.RETRIEVAL_METRICS)})")
    keep, chunks = int(keep), _chunks(who, chunks, "chunks of gallery rows")
    if not 0 <= keep <= H.RETRIEVAL_MAX_KEEP:
        raise ValueError(f"{who}: keep = {keep} neighbours (0 .. {H.RETRIEVAL_MAX_KEEP} are on the MI355X path)")
    loc = _retrieval_sets(who, "loc", loc)
    S, N, D = loc.shape
    if metric in ("w2", "skl"):
        if scale is None:
            raise ValueError(f"{who}: metric {metric!r} compares distributions and needs `scale`")
        scale = _retrieval_sets(who, "scale", scale, loc)
        if not bool((scale > 0).all()):
            raise ValueError(f"{who}: scale holds values that are not positive")
    else:
        scale = None      # (l2 and cosine read the means alone)
    if pairs is None:
        pairs = retrieval_pairs(S)
    pt = _retrieval_ints(who, "pairs", pairs, "an integer (P, 2) list of (query set, gallery set)")
    if pt.dim() != 2 or pt.shape[1] != 2 or not 1 <= pt.shape[0] <= H.RETRIEVAL_MAX_PAIRS:
        raise ValueError(f"{who}: pairs is {tuple(pt.shape)}; (P, 2) with 1 <= P <= {H.RETRIEVAL_MAX_PAIRS} pairs")
    if int(pt.min()) < 0 or int(pt.max()) >= S or bool((pt[:, 0] == pt[:, 1]).any()):
        raise ValueError(f"{who}: pairs must hold two different sets out of 0 .. {S - 1} per row")
    if match is not None:
        match = _retrieval_ints(who, "match", match, "an integer (N,) list of gallery rows, -1 for none")
        if tuple(match.shape) != (N,):
            raise ValueError(f"{who}: match is {tuple(match.shape)}; ({N},), one gallery row per query row")
        if int(match.min()) < -1 or int(match.max()) >= N:
            raise ValueError(f"{who}: match holds entries outside -1 .. {N - 1}")
    if loc.device.type != "cuda":
        raise ValueError(f"{who}: loc is on {loc.device}; the kernel runs on the MI355X (there is no host path)")
    dev, P = loc.device, pt.shape[0]
    pd = pt.to(device=dev, dtype=torch.int32).contiguous()
    md = None if match is None else match.to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(H.lib().mmvae_retrieval_ws_bytes(N, P, keep, chunks) // 8, dtype=torch.float64, device=dev)
    d_match = torch.empty(P, N, dtype=torch.float64, device=dev)
    less, equal = (torch.empty(P, N, dtype=torch.int32, device=dev) for _ in range(2))
    nn_d = torch.empty(P, N, keep, dtype=torch.float64, device=dev)
    nn_idx = torch.empty(P, N, keep, dtype=torch.int32, device=dev)
    _call("mmvae_retrieval_ranks", H.ptr(loc), H.ptr(scale), H.ptr(pd), H.ptr(md), H.ptr(ws) if ws.numel() else None,
          H.ptr(d_match), H.ptr(less), H.ptr(equal), H.ptr(nn_d) if keep else None, H.ptr(nn_idx) if keep else None, N, D, S, P,
          H.RETRIEVAL_METRICS[metric], keep, chunks, H.stream())
    return {"d_match": d_match, "less": less, "equal": equal, "nn_d": nn_d, "nn_idx": nn_idx,
            "pairs": [tuple(r) for r in pt.tolist()]}


def _retrieval_ks(who, ks):
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or len(set(ks)) != len(ks):
        raise ValueError(f"{who}: ks = {ks} (different positive numbers of neighbours)")
    return ks


def retrieval_summary(less, equal, ks=(1, 5, 10), n_gallery=None):
    """Recall@k, median rank and their kin from the `less` and `equal` counts of retrieval_ranks; on the host.
    PESSIMISTIC ranks: rank = 1 + less + equal -- a gallery row exactly as near as the partner is counted as if it were nearer,
    so a tie never counts as a hit: N identical embeddings score rank N, not 1, and collapsed posteriors score at the far end
    rather than as perfect retrieval.  Rows without a partner (less < 0) are left out.  `n_gallery`: the gallery's rows
    (default: the number of query rows).  Per pair (one dict for (N,) counts, a list of P dicts for (P, N)):
      "recall@k" = share of rows with rank <= k, "chance@k" = min(k / n_gallery, 1), "median_rank", "mean_rank", "mrr" = mean
      1 / rank, "normalised_rank" = mean (rank - 1) / (n_gallery - 1) (0 best, 1 worst, 0.5 at chance; 0 for one gallery
      row), "tied_rows" = rows with equal > 0, "n" = rows with a partner (NaN everywhere but the chances when 0)."""
    who = "retrieval_summary"
    ks = _retrieval_ks(who, ks)
    less = _retrieval_ints(who, "less", less, "the integer (N,) or (P, N) counts of retrieval_ranks").numpy()
    equal = _retrieval_ints(who, "equal", equal, "the integer (N,) or (P, N) counts of retrieval_ranks").numpy()
    if less.shape != equal.shape or less.ndim not in (1, 2) or less.shape[-1] < 1:
        raise ValueError(f"{who}: less is {less.shape}, equal {equal.shape}; the (N,) or (P, N) counts of retrieval_ranks")
    if bool(((less < 0) != (equal < 0)).any()):
        raise ValueError(f"{who}: less and equal disagree on the rows without a partner")
    Ng = less.shape[-1] if n_gallery is None else int(n_gallery)
    most = int((less.astype(np.int64) + equal).max())
    if Ng < 1 or most >= Ng:
        raise ValueError(f"{who}: n_gallery = {Ng} rows for a row with less + equal = {most} other rows")

    def one(l, e):
        has = l >= 0
        rank = (1 + l[has].astype(np.int64) + e[has].astype(np.int64)).astype(np.float64)
        n = int(has.sum())
        out = {"n": n, "tied_rows": int((e[has] > 0).sum())}
        for k in ks:
            out[f"recall@{k}"] = float((rank <= k).mean()) if n else float("nan")
            out[f"chance@{k}"] = min(k / Ng, 1.0)
        out["median_rank"] = float(np.median(rank)) if n else float("nan")
        out["mean_rank"] = float(rank.mean()) if n else float("nan")
        out["mrr"] = float((1.0 / rank).mean()) if n else float("nan")
        out["normalised_rank"] = (float(((rank - 1.0) / (Ng - 1)).mean()) if Ng > 1 else 0.0) if n else float("nan")
        return out

    return one(less, equal) if less.ndim == 1 else [one(l, e) for l, e in zip(less, equal)]


def retrieval_label_precision(nn_idx, labels_q, labels_g, ks=(1, 5, 10)):
    """Do a query's nearest gallery rows carry its label?  nn_idx (N, keep): the neighbour lists of one pair from
    retrieval_ranks (-1: an empty slot); labels_q (N,), labels_g (gallery rows,) integers; every k of `ks` <= keep.  On the
    host -> {k: {"precision": the mean over the queries of the share of the (filled) first k slots that carry the query's
    label, "hit": the share of queries with at least one such row among them}}."""
    who = "retrieval_label_precision"
    ks = _retrieval_ks(who, ks)
    idx = _retrieval_ints(who, "nn_idx", nn_idx, "the integer (N, keep) neighbour lists of one pair").numpy()
    lq = _retrieval_ints(who, "labels_q", labels_q, "an integer (N,) list, one label per query row").numpy()
    lg = _retrieval_ints(who, "labels_g", labels_g, "an integer list, one label per gallery row").numpy()
    if idx.ndim != 2 or lq.shape != (idx.shape[0],) or lg.ndim != 1 or lg.shape[0] < 1:
        raise ValueError(f"{who}: nn_idx is {idx.shape}, labels_q {lq.shape}, labels_g {lg.shape}; (N, keep), (N,) and (gallery "
                         f"rows,)")
    if max(ks) > idx.shape[1]:
        raise ValueError(f"{who}: ks = {ks} for lists of keep = {idx.shape[1]} neighbours")
    if idx.size and (int(idx.min()) < -1 or int(idx.max()) >= lg.shape[0]):
        raise ValueError(f"{who}: nn_idx holds entries outside -1 .. {lg.shape[0] - 1}")
    filled = idx >= 0
    if not bool(filled[:, 0].all()):
        raise ValueError(f"{who}: a query has no neighbour at all")
    same = filled & (lg[np.where(filled, idx, 0)] == lq[:, None])
    out = {}
    for k in ks:
        share = same[:, :k].sum(1) / filled[:, :k].sum(1)
        out[k] = {"precision": float(share.mean()), "hit": float(same[:, :k].any(1).mean())}
    return out
