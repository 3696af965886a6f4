"""The training path: torch.autograd.Function wrappers around the C-ABI kernels, the optimiser calls, noise and the input
expanders (host plumbing only) -- and the one public namespace of every kernel wrapper.

The forward-only evaluation metrics live in the package `metrics`, one module per kernel file (metrics/loglik.py wraps
csrc/loglik.hip, and so on); the block at the end of this file imports their public names, so callers, the documents and
the tests say `ops.<name>` for a metric as for a layer.  The C call itself (`H.call`) and its counter belong to hipops.

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
import math
import os

import torch
from torch.autograd import Function

from . import hipops as H

_DACT = {H.ACT_NONE: H.EP_NONE, H.ACT_SILU: H.EP_MUL_SILU_GRAD, H.ACT_RELU: H.EP_MUL_RELU_MASK,
         H.ACT_GELU: H.EP_MUL_GELU_GRAD}

CALLS = H.CALLS      # (the counter of H.call: the same list)


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
        H.call("mmvae_linear_bwd_weight_batch", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())

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
        # x, dy: allocated on the chain's stream, read on the other one
        StreamPlan.hand([t for j in cls.cw_jobs for t in j[:2]], side, after=ev)
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
        H.call("mmvae_conv_wgrad_batch", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())

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
                H.call("mmvae_reduce_segments_lincomb", ctypes.byref(t), ctypes.byref(rp), flat, H.ptr(out), n, B, k,
                       H.stream())
                tail["done"] = True
            else:
                H.call("mmvae_reduce_segments", ctypes.byref(t), H.stream())
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
        H.call("mmvae_debug_timestamp", cls.buf.data_ptr() + 8 * i, H.stream())


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

    @staticmethod
    def hand(tensors, to, after=None):
        """THE way a tensor crosses streams: kernels queued on stream `to` from here on read `tensors`, which another
        stream allocated.  `after` (a stream or an event: what produced them): `to` first waits for it.  Every CUDA tensor
        is then registered with `to` -- without that the caching allocator hands its block to the allocating stream again
        as soon as the host drops the last reference, whatever `to` still has queued.  None entries, CPU tensors and a
        `to` of None are ignored.  (record_stream registers the tensor's STORAGE: a view stands for its whole block.)"""
        if to is None:
            return
        if after is not None and after != to:
            (to.wait_event if isinstance(after, torch.cuda.Event) else to.wait_stream)(after)
        for t in tensors:
            if t is not None and t.is_cuda:
                t.record_stream(to)


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
    H.call("mmvae_dropout_advance", H.ptr(state), int(slot), H.stream())


def dropout_advance_many(states):
    """dropout_advance(st, 0) for every state tensor in `states` (distinct towers) in one launch"""
    arr = (ctypes.c_void_p * len(states))(*[H.ptr(t) for t in states])
    H.call("mmvae_dropout_advance_many", ctypes.cast(arr, ctypes.c_void_p), len(states), H.stream())


def dropout_mask(drop, n):
    out = torch.empty(n, device=drop.state.device)
    H.call("mmvae_dropout_mask", drop.c(), H.ptr(out), n, H.stream())
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
        H.call("mmvae_conv2d_k4s2_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), B, Cin, Cout, Hin, in_act,
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
            H.call("mmvae_conv2d_k4s2_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
                   B, Cin, Cout, Hout, in_act, acc, H.stream())
        else:
            H.call("mmvae_conv2d_k4s2_wgrad", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), H.ptr(ws), B, Cin, Cout, Hout,
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
        H.call("mmvae_convT2d_k4s2_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), B, Cin, Cout, Hin, in_act,
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
            H.call("mmvae_sigmoid_clamp_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
            dy = dl
        elif out_ep == H.EP_SIGMOID:
            dl = torch.empty_like(dy)
            H.call("mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
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
        H.call("mmvae_convT2d_k4s2_dgrad", H.ptr(dy), H.ptr(w), H.ptr(x) if ep else None, H.ptr(dx), B, Cin, Cout, Hin, ep,
               H.stream())
        if go is not None:
            go()
    elif need_dx:       # input- and weight-gradient workgroups in ONE launch
        dx = torch.empty_like(x)
        H.call("mmvae_convT2d_k4s2_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
               B, Cin, Cout, Hin, in_act, acc, H.stream())
    else:
        H.call("mmvae_convT2d_k4s2_wgrad", H.ptr(x), H.ptr(dy), H.ptr(dw), H.ptr(db), H.ptr(ws), B, Cin, Cout, Hin,
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
        H.call("mmvae_convT3_bce_seeded", H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(target), H.ptr(row), H.ptr(dl), H.ptr(part),
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
        H.call("mmvae_sigmoid_clamp_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
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
            H.call("mmvae_bce_rowsum_seeded", H.ptr(y_raw), H.ptr(target), H.ptr(row), cs.value, H.ptr(dl), B, F_,
                   H.stream())
            ctx.seeded = (cs.seed.data_ptr(), dl)
        else:
            H.call("mmvae_bce_rowsum_fwd", H.ptr(y_raw), H.ptr(target), H.ptr(row), B, F_, trows, H.stream())
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
        H.call("mmvae_bce_sigmoid_clamp_bwd", H.ptr(y), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(dl), B, y.numel() // B,
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
        H.call("mmvae_convT2d_generic_fwd" if transposed else "mmvae_conv2d_generic_fwd", H.ptr(x), H.ptr(w), H.ptr(b),
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
            H.call("mmvae_sigmoid_clamp_bwd" if out_ep == H.EP_SIGMOID_CLAMP else "mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y),
                   H.ptr(dl), dy.numel(), H.stream())
            dy = dl
        dw, db, acc_w, ret_w, ret_b = _grad_dst(w, gw, gb, has_b, Cout)
        pre = "mmvae_convT2d_generic" if transposed else "mmvae_conv2d_generic"
        H.call(pre + "_wgrad", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), B, Cin, Cout, Hin, Win, K, stride, pad, in_act,
               acc_w, H.stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ep = _DACT[in_act]
            H.call(pre + "_dgrad", H.ptr(dy), H.ptr(w), H.ptr(x) if ep else None, H.ptr(dx), B, Cin, Cout, Hin, Win, K,
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
            H.call("mmvae_linear_fwd", H.ptr(x), H.ptr(w), H.ptr(b), None, H.ptr(y), M, N, K, K, in_act, out_ep, H.stream())
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
            H.call("mmvae_linear_bwd_data", H.ptr(dy), H.ptr(w), aux, H.ptr(dx), M, N, K, ep, 0, H.stream())
            GradReducer.tw_park((dy.view(M, N), x.view(M, K), w, True, gw, gb))
            del kadd
            return dx, ret_w, ret_b, None, None, None, None, None, None
        if need_dx and defer and nz == 1 and radd is None and GradReducer.dw_later(x.device) and \
                lib.mmvae_linear_bwd_weight_splits(M, N, K) == 1:
            # the captured one-GPU MoPoE step, a Linear of the decoder that shares the fusion's stream: only the DATA
            # gradient sits on the critical chain decoder -> fusion -> encoders; the weight gradients of all such layers
            # follow in ONE launch behind the fusion's backward (GradReducer.flush_dw)
            H.call("mmvae_linear_bwd_data", H.ptr(dy), H.ptr(w), aux, H.ptr(dx), M, N, K, ep, 0, H.stream())
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
            H.call("mmvae_linear_bwd", H.ptr(dy), H.ptr(x), H.ptr(w), aux, H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(ws),
                   M, N, K, K, in_act, ep, acc, H.stream())
        else:
            GradReducer.writes(x.device, *direct)
            H.call("mmvae_linear_bwd_weight", H.ptr(dy), H.ptr(x), H.ptr(dw), H.ptr(db), H.ptr(ws), M, N, K, K, in_act, acc,
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
        H.call("mmvae_sigmoid_bwd", H.ptr(dy), H.ptr(y), H.ptr(dl), dy.numel(), H.stream())
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
        H.call("mmvae_gemm_f32", H.ptr(x), H.ptr(w), None, None, H.ptr(y), None, None, M, N, K, K, 1, N, 1, N, in_act,
               H.ACT_NONE, H.EP_NONE, 0, 1, H.stream())
        if b is not None:
            H.call("mmvae_bias_group_add", H.ptr(y), H.ptr(b), M, C, G, H.stream())
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
            H.call("mmvae_gemm_f32", H.ptr(dy), H.ptr(w), None, H.ptr(x) if ep else None, H.ptr(dx), None, None, M, K, N,
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
        H.call("mmvae_gemm_f32", H.ptr(x), H.ptr(dy), None, None, H.ptr(dw), None, H.ptr(ws), K, N, M, 1, K, N, 1, N,
               in_act, H.ACT_NONE, H.EP_NONE, H.ACC_DEFER if defer else acc_w, want, H.stream())
        if defer:
            GradReducer.add(ws.data_ptr(), dw, nz, K * N, K * N)
        ret_b = None
        if has_b:
            nbw = lib.mmvae_bias_group_ws_floats(M, C)
            if _defer(gb):
                bws = GradReducer.alloc(nbw, x.device)
                H.call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(gb), H.ptr(bws), M, C, G, H.ACC_DEFER, H.stream())
                GradReducer.add(bws.data_ptr(), gb, lib.mmvae_bias_group_parts(M), C, C)
            elif gb is not None:
                bws = torch.empty(nbw, device=x.device)
                GradReducer.writes(x.device, gb)
                H.call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(gb), H.ptr(bws), M, C, G, 1, H.stream())
            else:
                ret_b = torch.empty(C, device=x.device)
                bws = torch.empty(nbw, device=x.device)
                H.call("mmvae_bias_group_grad", H.ptr(dy), H.ptr(ret_b), H.ptr(bws), M, C, G, 0, H.stream())
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
        H.call("mmvae_avgpool_fwd", H.ptr(x), H.ptr(y), B, HW, C, in_act, H.stream())
        ctx.save_for_backward(x)
        ctx.cfg = (B, HW, C, in_act)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, HW, C, in_act = ctx.cfg
        dx = torch.empty_like(x)
        H.call("mmvae_avgpool_bwd", H.ptr(H.f32c(dy)), H.ptr(x), H.ptr(dx), B, HW, C, in_act, H.stream())
        return dx, None, None, None


class HeadSoftmax(Function):
    """h (B,2D) = [mu | u]  ->  [mu | softmax(u)+1e-6]   (VaeComponent.process_output, models/encoders.py:49-54)"""

    @staticmethod
    def forward(ctx, h):
        assert h.is_contiguous() and h.dtype == torch.float32
        B, D2 = h.shape
        H.call("mmvae_head_softmax_fwd", H.ptr(h), B, D2 // 2, H.stream())   # in place on the fresh linear output
        ctx.mark_dirty(h)
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, dh):
        (out,) = ctx.saved_tensors
        # h feeds nothing but this op, so the incoming gradient buffer is exclusively ours: transform it in place
        dh = H.f32c(dh)
        B, D2 = out.shape
        H.call("mmvae_head_softmax_bwd", H.ptr(out), H.ptr(dh), B, D2 // 2, H.stream())
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
        H.call("mmvae_poe_reparam_kl_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(joint), H.ptr(kl), E, int(with_prior),
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
        dth, acc, ret = _theta_grad_dest(theta, gtheta, True)      # (a fresh tensor whether autograd wants it or not)
        ws = H.workspace(H.lib().mmvae_poe_ws_floats(B, D), dev)
        H.call("mmvae_poe_reparam_kl_bwd_acc", ctypes.byref(a), H.ptr(theta), H.ptr(dkl), H.ptr(dth), H.ptr(ws),
               _poe_ticket(dev), E,
               int(with_prior), n_z if dz is not None else 0, kl_mask, B, D, 2 * Dtot, raw, acc, acc_packed, H.stream())
        return (ret, None, None, None, None, None, None, None, None, *(dpacked if ret_packed is None else ret_packed),
                *([None] * ctx.n_eps_in))


# ---- plumbing under the four single-pass fusions (TcFusion, JsFusion, MixPriorFusion, MmPlusFusion) -------------------
def _fusion_inputs(theta, eps, packed, eps_per_expert=False):
    """float32 contiguous inputs and their shared shape checks: E heads (B, 2 D) = [mu_e | lv_e], theta of D numbers, eps
    (B,D) or, `eps_per_expert`, (E,B,D) -> (packed, theta, eps, E, B, D, device)"""
    packed = [H.f32c(t) for t in packed]
    theta, eps = H.f32c(theta), H.f32c(eps)
    E = len(packed)
    B, D2 = packed[0].shape
    D = D2 // 2
    assert all(p.shape == (B, D2) for p in packed) and theta.numel() == D
    assert eps.shape == ((E, B, D) if eps_per_expert else (B, D))
    return packed, theta, eps, E, B, D, packed[0].device


def _head_tables(a, packed, D, dpacked=None):
    """the pointer table `a`: mu / lv of every head and, backward, dmu / dlv of its gradient tensor -> a.  (No more than
    the table holds: a longer list reaches the kernel's entry as its E, which refuses it.)"""
    for e, p in enumerate(packed[:H.MAX_EXPERTS]):
        a.mu[e] = p.data_ptr()
        a.lv[e] = p.data_ptr() + 4 * D
        if dpacked is not None:
            a.dmu[e] = dpacked[e].data_ptr()
            a.dlv[e] = dpacked[e].data_ptr() + 4 * D
    return a


def _upstream(g):
    """an upstream gradient for a kernel: an absent one goes in as NULL and the kernel takes it as zeros"""
    return H.f32c(g) if g is not None else None


def _theta_grad_dest(theta, gtheta, wanted):
    """where a fusion's backward pass leaves the prior parameter's gradient -> (dth, acc, ret): added to the preset view
    `gtheta`; else written to a fresh tensor that goes back to autograd; else, not `wanted`, nowhere (dth None: the fold
    is not launched)"""
    if gtheta is not None:
        GradReducer.writes(theta.device, gtheta)
        return gtheta, 1, None
    if not wanted:
        return None, 0, None
    ret = torch.empty_like(theta)
    return ret, 0, ret


def _fusion_ws(ws_floats, B, D, dev, *more):
    """the backward kernel's partial prior-gradient rows; ws_floats: the name of the op's mmvae_*_ws_floats (`more`: its
    arguments behind B and D)"""
    return H.workspace(getattr(H.lib(), ws_floats)(B, D, *more), dev)


class TcFusion(Function):
    """Product of experts (no prior expert) -> ONE reparameterised sample -> KL of the joint to the prior (row E) and to
    every expert (rows 0 .. E-1): MVTCAE's latent op (csrc/tcfusion.hip).  packed[e]: (B, 2 D) = [mu_e | lv_e] head
    outputs.  Returns joint (2,B,D) [not differentiable], kl (E+1,B), z (B,D)."""

    @staticmethod
    def forward(ctx, theta, gtheta, raw, eps, *packed):
        packed, theta, eps, E, B, D, dev = _fusion_inputs(theta, eps, packed)
        joint = torch.empty(2, B, D, device=dev)
        kl = torch.empty(E + 1, B, device=dev)
        z = torch.empty(B, D, device=dev)
        a = _head_tables(H.TcFwdArgs(), packed, D)
        H.call("mmvae_tc_fusion_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps), H.ptr(joint), H.ptr(kl), H.ptr(z), E, B, D,
               2 * D, int(bool(raw)), H.stream())
        ctx.save_for_backward(theta, eps, *packed)
        ctx.cfg = (gtheta, E, B, D, int(bool(raw)))
        ctx.mark_non_differentiable(joint)
        ctx.set_materialize_grads(False)
        return joint, kl, z

    @staticmethod
    def backward(ctx, _dj, dkl, dz):
        gtheta, E, B, D, raw = ctx.cfg
        theta, eps, *packed = ctx.saved_tensors
        dpacked = [torch.empty_like(p) for p in packed]
        a = _head_tables(H.TcBwdArgs(), packed, D, dpacked)
        dth, acc, ret = _theta_grad_dest(theta, gtheta, ctx.needs_input_grad[0])
        ws = _fusion_ws("mmvae_tc_fusion_ws_floats", B, D, theta.device)
        dz, dkl = _upstream(dz), _upstream(dkl)
        H.call("mmvae_tc_fusion_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps), H.ptr(dz), H.ptr(dkl), H.ptr(dth),
               H.ptr(ws), E, B, D, 2 * D, raw, acc, H.stream())
        return (ret, None, None, None, *dpacked)


def tc_fusion(theta, packed, eps, gtheta=None, raw=False):
    """-> joint (2,B,D), kl (E+1,B), z (B,D) of the total-correlation fusion (TcFusion); gtheta: the prior parameter's
    preset gradient view, which the backward pass then adds to; raw: packed = [mu | raw logvar-head output]"""
    return TcFusion.apply(theta, gtheta, raw, eps, *packed)


class JsFusion(Function):
    """Weighted geometric mean of the E experts N(mu_e, sigma = lv_e) and the prior (the dynamic prior) -> KL of each of
    the E + 1 to it (rows 0 .. E-1 the experts', row E the prior's) -> ONE reparameterised sample per row from expert
    sel[b]: mmJSD's latent op (csrc/jsfusion.hip).  packed[e]: (B, 2 D) = [mu_e | lv_e] head outputs.  Returns prior
    (2,B,D) = [mean, scale] [not differentiable], kl (E+1,B), z (B,D)."""

    @staticmethod
    def forward(ctx, theta, gtheta, raw, weights, sel, eps, *packed):
        packed, theta, eps, E, B, D, dev = _fusion_inputs(theta, eps, packed)
        assert sel.dtype == torch.int32 and sel.shape == (B,) and sel.is_contiguous() and len(weights) == E + 1
        prior = torch.empty(2, B, D, device=dev)
        kl = torch.empty(E + 1, B, device=dev)
        z = torch.empty(B, D, device=dev)
        a = _head_tables(H.TcFwdArgs(), packed, D)
        w = (H.c_f * (E + 1))(*weights)
        H.call("mmvae_js_fusion_fwd", ctypes.byref(a), w, H.ptr(theta), H.ptr(eps), H.ptr(sel), H.ptr(prior), H.ptr(kl),
               H.ptr(z), E, B, D, 2 * D, int(bool(raw)), H.stream())
        ctx.save_for_backward(theta, eps, sel, *packed)
        ctx.cfg = (gtheta, E, B, D, int(bool(raw)), w)
        ctx.mark_non_differentiable(prior)
        ctx.set_materialize_grads(False)
        return prior, kl, z

    @staticmethod
    def backward(ctx, _dp, dkl, dz):
        gtheta, E, B, D, raw, w = ctx.cfg
        theta, eps, sel, *packed = ctx.saved_tensors
        dpacked = [torch.empty_like(p) for p in packed]
        a = _head_tables(H.TcBwdArgs(), packed, D, dpacked)
        dth, acc, ret = _theta_grad_dest(theta, gtheta, ctx.needs_input_grad[0])
        ws = _fusion_ws("mmvae_js_fusion_ws_floats", B, D, theta.device)
        dz, dkl = _upstream(dz), _upstream(dkl)
        H.call("mmvae_js_fusion_bwd", ctypes.byref(a), w, H.ptr(theta), H.ptr(eps), H.ptr(sel), H.ptr(dz), H.ptr(dkl),
               H.ptr(dth), H.ptr(ws), E, B, D, 2 * D, raw, acc, H.stream())
        return (ret, None, None, None, None, None, *dpacked)


def js_fusion(theta, packed, eps, sel, weights, gtheta=None, raw=False):
    """-> prior (2,B,D), kl (E+1,B), z (B,D) of the Jensen-Shannon fusion (JsFusion).  sel: the expert every row's sample is
    drawn from, int32 (B,): a list or a CPU tensor is checked against [0, E) here and moved to the device, a device tensor
    is taken as is (the kernel compares indices: a value no expert has gives a zero row).  weights: pi_0 .. pi_E, the
    last one the prior's; gtheta, raw: as tc_fusion"""
    E, dev = len(packed), packed[0].device
    weights = [float(x) for x in weights]
    if len(weights) != E + 1:
        raise ValueError(f"js_fusion: {len(weights)} weights for {E} experts and the prior ({E + 1} wanted)")
    if not (torch.is_tensor(sel) and sel.is_cuda):
        sel = torch.as_tensor(sel).reshape(-1)
        if sel.dtype.is_floating_point or sel.dtype == torch.bool:
            raise ValueError(f"js_fusion: sel holds expert indices, not {sel.dtype}")
        if sel.numel() and not (0 <= int(sel.min()) and int(sel.max()) < E):
            raise ValueError(f"js_fusion: sel values must lie in [0, {E}): found [{int(sel.min())}, {int(sel.max())}]")
        sel = sel.to(device=dev, dtype=torch.int32)
    elif sel.dtype != torch.int32:
        sel = sel.to(torch.int32)
    return JsFusion.apply(theta, gtheta, raw, weights, sel.contiguous(), eps, *packed)


class MixPriorFusion(Function):
    """ONE reparameterised sample from EVERY expert N(mu_e, sigma = lv_e) -> the one-sample estimate of every expert's KL
    to the uniform mixture of all E (rows 0 .. E-1) and its closed-form KL to the prior (rows E .. 2E-1) -> the
    responsibilities: the MMVM VAE's latent op (csrc/mixprior.hip).  packed[e]: (B, 2 D) = [mu_e | lv_e] head outputs, eps
    (E,B,D).  Returns kl (2E,B), resp (E,E,B) [not differentiable], z_0 .. z_{E-1} (B,D) each: E outputs, so that every
    decoder's gradient arrives on its own (or as None) and goes to the kernel as it is."""

    @staticmethod
    def forward(ctx, theta, gtheta, raw, eps, *packed):
        packed, theta, eps, E, B, D, dev = _fusion_inputs(theta, eps, packed, eps_per_expert=True)
        kl = torch.empty(2 * E, B, device=dev)
        resp = torch.empty(E, E, B, device=dev)
        zs = [torch.empty(B, D, device=dev) for _ in range(E)]
        a = _head_tables(H.PoeFwdArgs(), packed, D)
        for e in range(min(E, H.MAX_EXPERTS)):
            a.eps[e] = eps.data_ptr() + 4 * e * B * D
            a.z[e] = zs[e].data_ptr()
        H.call("mmvae_mixprior_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(kl), H.ptr(resp), E, B, D, 2 * D, int(bool(raw)),
               H.stream())
        ctx.save_for_backward(theta, eps, resp, *packed)
        ctx.cfg = (gtheta, E, B, D, int(bool(raw)))
        ctx.mark_non_differentiable(resp)
        ctx.set_materialize_grads(False)
        return (kl, resp, *zs)

    @staticmethod
    def backward(ctx, dkl, _dresp, *dzs):
        gtheta, E, B, D, raw = ctx.cfg
        theta, eps, resp, *packed = ctx.saved_tensors
        dpacked = [torch.empty_like(p) for p in packed]
        a = _head_tables(H.PoeBwdArgs(), packed, D, dpacked)
        dkl, dzs = _upstream(dkl), [_upstream(g) for g in dzs]
        for e in range(E):
            a.eps[e] = eps.data_ptr() + 4 * e * B * D
            a.dz[e] = H.ptr(dzs[e])
        dth, acc, ret = _theta_grad_dest(theta, gtheta, ctx.needs_input_grad[0])
        ws = _fusion_ws("mmvae_mixprior_ws_floats", B, D, theta.device)
        H.call("mmvae_mixprior_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(resp), H.ptr(dkl), H.ptr(dth), H.ptr(ws), E, B, D,
               2 * D, raw, acc, H.stream())
        return (ret, None, None, None, *dpacked)


def mixprior_fusion(theta, packed, eps, gtheta=None, raw=False):
    """-> z (a tuple of E tensors (B,D), z[e] = mu_e + sigma_e eps[e]), kl (2E,B), resp (E,E,B) of the mixture-of-experts
    prior (MixPriorFusion).  eps: (E,B,D) standard-normal draws; gtheta, raw: as tc_fusion"""
    E = len(packed)
    if tuple(eps.shape) != (E, packed[0].shape[0], packed[0].shape[1] // 2):
        raise ValueError(f"mixprior_fusion: eps is {tuple(eps.shape)}; {E} experts of shape {tuple(packed[0].shape)} want "
                         f"({E}, {packed[0].shape[0]}, {packed[0].shape[1] // 2})")
    kl, resp, *zs = MixPriorFusion.apply(theta, gtheta, raw, eps, *packed)
    return tuple(zs), kl, resp


class MmPlusFusion(Function):
    """MMVAE+'s latent op, K = 1 (csrc/mmplus.hip).  packed[e]: (B, 2 W) = [mu_e | lv_e] head outputs of W = D + P columns
    per half, [0, D) the shared posterior, [D, W) the private one; eps_u (E,B,D), eps_w (E,B,P), eps_a (E,E,B,P) indexed
    [decoder][source].  Returns kl (3E,B) -- rows m: the one-sample KL of the shared posterior to the mixture of all E, rows
    E + m: its closed-form KL to the prior, rows 2E + m: the private posterior's to N(0, 1) --, resp (E,E,B) [not
    differentiable], and z_0 .. z_{E-1} (E B, W) each: decoder n's whole input batch, row block m = [u_m | w_m] if n == m,
    else [u_m | aux_scale eps_a[n][m]].  E outputs, so that every decoder's gradient arrives on its own (or as None)."""

    @staticmethod
    def forward(ctx, theta, gtheta, raw, D, aux_scale, eps_u, eps_w, eps_a, *packed):
        packed = [H.f32c(t) for t in packed]
        theta, eps_u, eps_w, eps_a = H.f32c(theta), H.f32c(eps_u), H.f32c(eps_w), H.f32c(eps_a)
        E, (B, W2), dev = len(packed), packed[0].shape, packed[0].device
        W = W2 // 2
        P = W - D
        assert all(p.shape == (B, W2) for p in packed) and theta.numel() == D
        assert eps_u.shape == (E, B, D) and eps_w.shape == (E, B, P) and eps_a.shape == (E, E, B, P)
        kl = torch.empty(3 * E, B, device=dev)
        resp = torch.empty(E, E, B, device=dev)
        zs = [torch.empty(E * B, W, device=dev) for _ in range(E)]
        a = _head_tables(H.MmPlusFwdArgs(), packed, W)
        for e in range(min(E, H.MAX_EXPERTS)):
            a.z[e] = zs[e].data_ptr()
        H.call("mmvae_mmplus_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps_u), H.ptr(eps_w), H.ptr(eps_a), float(aux_scale),
               H.ptr(kl), H.ptr(resp), E, B, D, P, 2 * W, int(bool(raw)), H.stream())
        ctx.save_for_backward(theta, eps_u, eps_w, resp, *packed)
        ctx.cfg = (gtheta, E, B, D, P, int(bool(raw)))
        ctx.mark_non_differentiable(resp)
        ctx.set_materialize_grads(False)
        return (kl, resp, *zs)

    @staticmethod
    def backward(ctx, dkl, _dresp, *dzs):
        gtheta, E, B, D, P, raw = ctx.cfg
        theta, eps_u, eps_w, resp, *packed = ctx.saved_tensors
        dpacked = [torch.empty_like(p) for p in packed]
        a = _head_tables(H.MmPlusBwdArgs(), packed, D + P, dpacked)
        dkl, dzs = _upstream(dkl), [_upstream(g) for g in dzs]
        for e in range(E):
            a.dz[e] = H.ptr(dzs[e])
        dth, acc, ret = _theta_grad_dest(theta, gtheta, ctx.needs_input_grad[0])
        ws = _fusion_ws("mmvae_mmplus_ws_floats", B, D, theta.device, P)
        H.call("mmvae_mmplus_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(eps_u), H.ptr(eps_w), H.ptr(resp), H.ptr(dkl),
               H.ptr(dth), H.ptr(ws), E, B, D, P, 2 * (D + P), raw, acc, H.stream())
        return (ret, None, None, None, None, None, None, None, *dpacked)


def mmplus_fusion(theta, packed, eps_u, eps_w, eps_a, D, aux_scale, gtheta=None, raw=False):
    """-> z (a tuple of E tensors (E B, W): every decoder's input batch), kl (3E,B), resp (E,E,B) of MMVAE+'s latent op
    (MmPlusFusion).  D: the number of shared columns of the W = packed[e].shape[1] / 2 (the rest are private); eps_u
    (E,B,D), eps_w (E,B,W-D), eps_a (E,E,B,W-D) standard-normal draws; aux_scale: the scale of the auxiliary cross prior;
    gtheta, raw: as tc_fusion"""
    E = len(packed)
    if E < 1:
        raise ValueError("mmplus_fusion: no heads")
    B, W2 = packed[0].shape
    D, aux_scale = int(D), float(aux_scale)
    P = W2 // 2 - D
    if W2 % 2 or any(tuple(p.shape) != (B, W2) for p in packed):
        raise ValueError(f"mmplus_fusion: heads of shapes {[tuple(p.shape) for p in packed]}: every head is (B, 2 W) = "
                         f"[mu | lv] with the same B and W")
    if D < 1 or P < 1:
        raise ValueError(f"mmplus_fusion: D = {D} shared of W = {W2 // 2} columns leaves P = {P} private: both must be >= 1")
    if theta.numel() != D:
        raise ValueError(f"mmplus_fusion: theta has {theta.numel()} elements; the D = {D} shared columns want {D}")
    for name, t, want in (("eps_u", eps_u, (E, B, D)), ("eps_w", eps_w, (E, B, P)), ("eps_a", eps_a, (E, E, B, P))):
        if tuple(t.shape) != want:
            raise ValueError(f"mmplus_fusion: {name} is {tuple(t.shape)}; {E} heads of shape {(B, W2)} with D = {D} want {want}")
    if not (math.isfinite(aux_scale) and aux_scale > 0):
        raise ValueError(f"mmplus_fusion: aux_scale = {aux_scale} must be finite and > 0")
    kl, resp, *zs = MmPlusFusion.apply(theta, gtheta, raw, D, aux_scale, eps_u, eps_w, eps_a, *packed)
    return tuple(zs), kl, resp


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
        H.call("mmvae_rows_fan_fwd", ctypes.byref(t), H.stream())
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
            H.call("mmvae_rows_fan_bwd", ctypes.byref(t), H.stream())
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
        H.call("mmvae_bce_rowsum_fwd", H.ptr(x_hat), H.ptr(target), H.ptr(row), B, F, B, H.stream())
        ctx.save_for_backward(x_hat, target)
        return row

    @staticmethod
    def backward(ctx, g):
        x_hat, target = ctx.saved_tensors
        B = x_hat.shape[0]
        F = x_hat.numel() // B
        dx = torch.empty_like(x_hat)
        H.call("mmvae_bce_rowsum_bwd", H.ptr(x_hat), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(dx), B, F, H.stream())
        return dx, None


class BceElem(Function):
    """elementwise bce (B,F) -- the literal ReconLoss.bce output"""

    @staticmethod
    def forward(ctx, x_hat, target):
        x_hat, target = H.f32c(x_hat), H.f32c(target)
        out = torch.empty_like(x_hat)
        H.call("mmvae_bce_elem_fwd", H.ptr(x_hat), H.ptr(target), H.ptr(out), x_hat.numel(), H.stream())
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
        H.call("mmvae_lprob_rowsum_fwd", H.ptr(loc), H.ptr(target), H.ptr(row), B, F_, trows, sc, lap, lap_rows,
               int(perm_c), H.stream())
        ctx.save_for_backward(loc, target)
        ctx.cfg = (sc, lap, lap_rows, B, F_, trows, int(perm_c), int(bool(logit_grad)))
        return row

    @staticmethod
    def backward(ctx, g):
        loc, target = ctx.saved_tensors
        sc, lap, lap_rows, B, F_, trows, perm_c, logit_grad = ctx.cfg
        d = torch.empty_like(loc)
        H.call("mmvae_lprob_rowsum_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), B, F_, trows, sc, lap,
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
        H.call("mmvae_optimal_sigma_fwd", H.ptr(loc), H.ptr(target), H.ptr(row), H.ptr(stats), H.ptr(ws), B, F_,
               H.stream())
        ctx.save_for_backward(loc, target, stats)
        return row

    @staticmethod
    def backward(ctx, g):
        loc, target, stats = ctx.saved_tensors
        B = loc.shape[0]
        d = torch.empty_like(loc)
        H.call("mmvae_optimal_sigma_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(stats), H.ptr(d), B,
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
        H.call("mmvae_lprob_elem_fwd", H.ptr(loc), H.ptr(target), H.ptr(out), loc.numel(), target.numel(), sc,
               int(bool(laplace)), H.stream())
        ctx.save_for_backward(loc, target)
        ctx.cfg = (sc, int(bool(laplace)))
        return out

    @staticmethod
    def backward(ctx, g):
        loc, target = ctx.saved_tensors
        g = g.to(torch.float64).contiguous()
        d = torch.empty_like(loc)
        H.call("mmvae_lprob_elem_bwd", H.ptr(loc), H.ptr(target), H.ptr(g), H.ptr(d), loc.numel(), target.numel(),
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
        H.call("mmvae_optimal_sigma_elem_fwd", H.ptr(loc), H.ptr(target), H.ptr(out), H.ptr(stats), H.ptr(ws), n,
               H.stream())
        ctx.save_for_backward(loc, target, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        loc, target, stats = ctx.saved_tensors
        n = loc.numel()
        d = torch.empty_like(loc)
        ws = torch.empty(H.lib().mmvae_optimal_sigma_ws_floats(1, n), device=loc.device)
        H.call("mmvae_optimal_sigma_elem_bwd", H.ptr(loc), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(stats), H.ptr(ws),
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
        H.call("mmvae_pointwise_rowsum_fwd", H.ptr(x), H.ptr(target), H.ptr(row), B, F_, trows, int(kind), H.stream())
        ctx.save_for_backward(x, target)
        ctx.cfg = (B, F_, trows, int(kind))
        return row

    @staticmethod
    def backward(ctx, g):
        x, target = ctx.saved_tensors
        B, F_, trows, kind = ctx.cfg
        d = torch.empty_like(x)
        H.call("mmvae_pointwise_rowsum_bwd", H.ptr(x), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), B, F_, trows, kind,
               H.stream())
        return d, None, None


class PointwiseElem(Function):
    """element-wise l1 / mse (the literal ReconLoss.l1 / .mse outputs)"""

    @staticmethod
    def forward(ctx, x, target, kind):
        x, target = H.f32c(x), H.f32c(target)
        out = torch.empty_like(x)
        H.call("mmvae_pointwise_elem", H.ptr(x), H.ptr(target), None, H.ptr(out), x.numel(), int(kind), H.stream())
        ctx.save_for_backward(x, target)
        ctx.kind = int(kind)
        return out

    @staticmethod
    def backward(ctx, g):
        x, target = ctx.saved_tensors
        d = torch.empty_like(x)
        H.call("mmvae_pointwise_elem", H.ptr(x), H.ptr(target), H.ptr(H.f32c(g)), H.ptr(d), x.numel(), ctx.kind,
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
        H.call("mmvae_add_pe_dropout_fwd", H.ptr(H.f32c(x)) if x is not None else None, H.ptr(pe), H.ptr(y), T, B, D,
               _dp(drop, y.numel()), H.stream())
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dy = H.f32c(dy)
        dx = torch.empty_like(dy)
        H.call("mmvae_dropout_act_bwd", H.ptr(dy), H.ptr(dy), H.ptr(dx), dy.numel(), H.ACT_NONE,
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
            H.call("mmvae_ce_over_time_seeded", H.ptr(logits), H.ptr(target), H.ptr(row), cs.value, H.ptr(dl), B, T, V,
                   H.stream())
            ctx.seeded = (cs.seed.data_ptr(), dl)
        else:
            H.call("mmvae_ce_over_time_fwd", H.ptr(logits), H.ptr(target), H.ptr(loss), H.ptr(row), B, T, V, trows,
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
        H.call("mmvae_ce_over_time_bwd", H.ptr(logits), H.ptr(target), H.ptr(g) if ctx.per_v else None,
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
        H.call("mmvae_lincomb_rowptrs_fwd", ctypes.byref(rp), flat, H.ptr(out), du, n, B, k, H.stream())
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
        H.call("mmvae_lincomb_rowptrs_bwd", ctypes.byref(gp), flat, ctypes.byref(dp), n, B, k, H.stream())
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
        H.call("mmvae_normal_logratio_fwd", H.ptr(packed_r), H.ptr(packed_o), H.ptr(z), H.ptr(lw), B, D2 // 2,
               H.stream())
        ctx.save_for_backward(packed_r, z)
        return lw

    @staticmethod
    def backward(ctx, g):
        packed_r, z = ctx.saved_tensors
        B, D2 = packed_r.shape
        d = torch.empty_like(packed_r)
        H.call("mmvae_normal_logratio_bwd", H.ptr(packed_r), H.ptr(z), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2,
               H.stream())
        return d, None, None


class ExpMul(Function):
    """exp(lw) * r"""

    @staticmethod
    def forward(ctx, lw, r):
        lw, r = H.f32c(lw), H.f32c(r)
        out = torch.empty_like(r)
        H.call("mmvae_expmul_fwd", H.ptr(lw), H.ptr(r), H.ptr(out), r.numel(), H.stream())
        ctx.save_for_backward(lw, r)
        return out

    @staticmethod
    def backward(ctx, g):
        lw, r = ctx.saved_tensors
        dlw, dr = torch.empty_like(lw), torch.empty_like(r)
        H.call("mmvae_expmul_bwd", H.ptr(lw), H.ptr(r), H.ptr(H.f32c(g)), H.ptr(dlw), H.ptr(dr), r.numel(), H.stream())
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
        H.call("mmvae_moe_elbo_fwd", H.ptr(V), flat, H.ptr(kld), H.ptr(out), n, M, B, float(beta), H.stream())
        ctx.save_for_backward(out)
        ctx.cfg = (flat, n, M, B, float(beta), tuple(kld.shape))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        flat, n, M, B, beta, kshape = ctx.cfg
        drows = torch.empty(n, B, device=out.device)
        dkld = torch.empty(kshape, device=out.device)
        H.call("mmvae_moe_elbo_bwd", H.ptr(H.f32c(g).reshape(1)), H.ptr(out), flat, H.ptr(drows), H.ptr(dkld), n, M, B,
               beta, H.stream())
        return (dkld, None, None, None, *[drows[i] for i in range(n)])


class LaplaceLogRatio(Function):
    """NormalLogRatio under Laplace posteriors (`prior: laplace`, models/mmvae_models.py:56-62)"""

    @staticmethod
    def forward(ctx, packed_r, packed_o, z):
        packed_r, packed_o, z = H.f32c(packed_r), H.f32c(packed_o), H.f32c(z)
        B, D2 = packed_r.shape
        lw = torch.empty(B, device=z.device)
        H.call("mmvae_laplace_logratio_fwd", H.ptr(packed_r), H.ptr(packed_o), H.ptr(z), H.ptr(lw), B, D2 // 2,
               H.stream())
        ctx.save_for_backward(packed_r, z)
        return lw

    @staticmethod
    def backward(ctx, g):
        packed_r, z = ctx.saved_tensors
        B, D2 = packed_r.shape
        d = torch.empty_like(packed_r)
        H.call("mmvae_laplace_logratio_bwd", H.ptr(packed_r), H.ptr(z), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2,
               H.stream())
        return d, None, None


class KlLaplaceNormal(Function):
    """kl[b] = sum_d KL(Laplace(mu, s) || N(0, 1)) for packed (B, 2D) = [mu | s]"""

    @staticmethod
    def forward(ctx, packed):
        packed = H.f32c(packed)
        B, D2 = packed.shape
        kl = torch.empty(B, device=packed.device)
        H.call("mmvae_kl_laplace_normal_fwd", H.ptr(packed), H.ptr(kl), B, D2 // 2, H.stream())
        ctx.save_for_backward(packed)
        return kl

    @staticmethod
    def backward(ctx, g):
        (packed,) = ctx.saved_tensors
        B, D2 = packed.shape
        d = torch.empty_like(packed)
        H.call("mmvae_kl_laplace_normal_bwd", H.ptr(packed), H.ptr(H.f32c(g)), H.ptr(d), B, D2 // 2, H.stream())
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
        H.call("mmvae_moe_ksample_fwd", ctypes.byref(a), H.ptr(theta), H.ptr(lat), H.ptr(pi), M, K, B, D, float(beta),
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
        H.call("mmvae_moe_ksample_bwd", ctypes.byref(a), H.ptr(theta), H.ptr(dlat), H.ptr(pi), H.ptr(rows), M, K, B, D,
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
        H.call("mmvae_dreg_loss_fwd", H.ptr(lat), ctypes.byref(t), H.ptr(out), M, K, B, H.stream())
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
        H.call("mmvae_dreg_loss_bwd", H.ptr(out), H.ptr(g), ctypes.byref(t), H.ptr(dlat), M, K, B, H.stream())
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
        H.call("mmvae_iwae_loss_fwd", H.ptr(lat), ctypes.byref(t), H.ptr(out), M, K, B, H.stream())
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
        H.call("mmvae_iwae_loss_bwd", H.ptr(lat), H.ptr(out), H.ptr(g), ctypes.byref(t), H.ptr(dlat), M, K, B, H.stream())
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
        H.call("mmvae_embed_pe_fwd", H.ptr(onehot), H.ptr(emb), H.ptr(pe), H.ptr(x), B, T, V, mode, B0, _dp(drop, x.numel()),
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
            H.call("mmvae_embed_pe_bwd", H.ptr(onehot), H.ptr(dx), None, H.ptr(ws), B, T, V, mode, B0, H.ACC_DEFER, dpc,
                   H.stream())
            GradReducer.add(ws.data_ptr(), de, H.lib().mmvae_embed_bwd_rows(B, T, V), 4, 4)
        else:
            ws = H.workspace(nws, dx.device)
            H.call("mmvae_embed_pe_bwd", H.ptr(onehot), H.ptr(dx), H.ptr(de), H.ptr(ws), B, T, V, mode, B0, acc, dpc,
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
        H.call("mmvae_attn_fwd", p, p + 4 * E, p + 8 * E, H.ptr(kpm), H.ptr(out), H.ptr(probs), L, L, N, nhead, hd, E3,
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
        H.call("mmvae_attn_bwd", p, p + 4 * E, p + 8 * E, H.ptr(probs), H.ptr(dout), d, d + 4 * E, d + 8 * E, L, L, N,
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
    H.call("mmvae_linear_bwd_weight", H.ptr(dy2), H.ptr(x2), H.ptr(dw), H.ptr(db), H.ptr(ws), M, N, K, K, x_act, acc,
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
    H.call("mmvae_txt_wgrad", ctypes.cast(arr, ctypes.c_void_p), len(jobs), H.stream())
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
        H.call("mmvae_txt_layer_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(mem) if dec else None, H.ptr(y), ctypes.byref(w),
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
            H.call("mmvae_linear_bwd", H.ptr(dy), H.ptr(z), H.ptr(hw), None, H.ptr(dz), H.ptr(hgw), H.ptr(hgb),
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
        H.call("mmvae_txt_layer_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), H.ptr(dmem), ctypes.byref(w),
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
                H.call("mmvae_proj32_ln_fwd", H.ptr(xin), H.ptr(pw), H.ptr(pb), H.ptr(r), H.ptr(gamma), H.ptr(beta), H.ptr(y),
                       H.ptr(xhat), H.ptr(rstd), rows, _dp(drop, x.numel()), H.stream())
            else:      # the Linear after all (its output was never computed), then the plain LayerNorm below
                H.call("mmvae_linear_fwd", H.ptr(xin), H.ptr(pw), H.ptr(pb), None, H.ptr(x), rows, d, xin.shape[-1],
                       xin.shape[-1], H.ACT_NONE, H.EP_NONE, H.stream())
        if not fused:
            H.call("mmvae_layernorm_residual_fwd", H.ptr(x), H.ptr(r), H.ptr(gamma), H.ptr(beta), H.ptr(y), H.ptr(xhat),
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
            H.call("mmvae_layernorm_residual_bwd", H.ptr(dy), H.ptr(xhat), H.ptr(rstd), H.ptr(gamma), H.ptr(dsum),
                   H.ptr(dxd), None, None, H.ptr(ws), rows, d, H.ACC_DEFER, dpc, H.stream())
            nb = H.lib().mmvae_layernorm_bwd_rows(rows, d)
            GradReducer.add(ws.data_ptr(), dg, nb, d, 2 * d)
            GradReducer.add(ws.data_ptr() + 4 * d, dbt, nb, d, 2 * d)
        else:
            ws = H.workspace(nws, dy.device)
            H.call("mmvae_layernorm_residual_bwd", H.ptr(dy), H.ptr(xhat), H.ptr(rstd), H.ptr(gamma), H.ptr(dsum),
                   H.ptr(dxd), dg.data_ptr(), dbt.data_ptr(), H.ptr(ws), rows, d, acc, dpc, H.stream())
        dr = None
        if has_r and ctx.needs_input_grad[1]:
            if r_rows:
                dr = torch.empty(rshape, device=dy.device)
                H.call("mmvae_sum_over_time", H.ptr(dsum), H.ptr(dr), rows // r_rows, r_rows, d, H.stream())
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
        H.call("mmvae_mean_over_time_fwd", H.ptr(x), H.ptr(y), L, N, d, H.stream())
        ctx.shape = (L, N, d)
        return y

    @staticmethod
    def backward(ctx, dy):
        L, N, d = ctx.shape
        dy = H.f32c(dy)
        dx = torch.empty(L, N, d, device=dy.device)
        H.call("mmvae_mean_over_time_bwd", H.ptr(dy), H.ptr(dx), L, N, d, H.stream())
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
            H.call("mmvae_permute_mask_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(y), T, B, V, H.stream())
        else:
            H.call("mmvae_permute_mask_head_fwd", H.ptr(x), H.ptr(mask_u8), H.ptr(y), T, B, V, Tk, H.stream())
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
            H.call("mmvae_permute_mask_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), T, B, V, H.stream())
        else:
            H.call("mmvae_permute_mask_head_bwd", H.ptr(dy), H.ptr(mask_u8), H.ptr(dx), T, B, V, Tk, H.stream())
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
        H.call("mmvae_dropout_act_fwd", H.ptr(x), H.ptr(y), x.numel(), act, _dp(drop, x.numel()), H.stream())
        ctx.save_for_backward(x)
        ctx.cfg = (act, drop)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        act, drop = ctx.cfg
        dy = H.f32c(dy)
        dx = torch.empty_like(x)
        H.call("mmvae_dropout_act_bwd", H.ptr(dy), H.ptr(x), H.ptr(dx), x.numel(), act, drop.c() if drop else None,
               H.stream())
        return dx, None, None


class HeadBcastDropout(Function):
    """(N,E) -> (L,N,E) with per-(n, head, l) attention-weight dropout (length-1 memory cross-attention)"""

    @staticmethod
    def forward(ctx, v, L, nhead, drop):
        v = H.f32c(v)
        N, E = v.shape
        out = torch.empty(L, N, E, device=v.device)
        H.call("mmvae_head_bcast_dropout_fwd", H.ptr(v), H.ptr(out), L, N, nhead, E // nhead, _dp(drop, N * nhead * L),
               H.stream())
        ctx.cfg = (L, N, E, nhead, drop)
        return out

    @staticmethod
    def backward(ctx, dout):
        L, N, E, nhead, drop = ctx.cfg
        dout = H.f32c(dout)
        dv = torch.empty(N, E, device=dout.device)
        H.call("mmvae_head_bcast_dropout_bwd", H.ptr(dout), H.ptr(dv), L, N, nhead, E // nhead,
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
                H.call("mmvae_ffn32_prep_weights", H.ptr(w1), H.ptr(w2), H.ptr(wsplit), FF, H.stream())
            if ln is not None:
                r_, gamma_, beta_, ln_drop = ln
                r_ = H.f32c(r_)
                yln, xhat, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(M, device=x.device)
                H.call("mmvae_ffn32_fwd_b16_ln", H.ptr(x), H.ptr(wsplit), H.ptr(b1), H.ptr(b2), H.ptr(r_), H.ptr(gamma_),
                       H.ptr(beta_), H.ptr(yln), H.ptr(xhat), H.ptr(rstd), M, FF, _dp(drop, M * FF), _dp(ln_drop, M * 32),
                       H.stream())
                Ffn32.last_pre = (yln, xhat, rstd)
            else:
                H.call("mmvae_ffn32_fwd_b16", H.ptr(x), H.ptr(wsplit), H.ptr(b1), H.ptr(b2), H.ptr(y), M, FF,
                       _dp(drop, M * FF), H.stream())
        else:
            H.call("mmvae_ffn32_fwd", H.ptr(x), H.ptr(w1), H.ptr(b1), H.ptr(w2), H.ptr(b2), H.ptr(y), M, FF,
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
                H.call("mmvae_ffn32_bwd_b16", H.ptr(x), H.ptr(dy), H.ptr(wsplit), H.ptr(b1), H.ptr(dx_), H.ptr(ws_), H.ptr(rsplit),
                       H.ptr(kadd) if dx_ is not None else None, M, FF, dc, H.stream())
        else:
            rsplit = None

            def bwd(dx_, ws_):
                H.call("mmvae_ffn32_bwd", H.ptr(x), H.ptr(dy), H.ptr(w1), H.ptr(b1), H.ptr(w2),
                       H.ptr(dx_) if dx_ is not None else None, H.ptr(ws_) if ws_ is not None else None, M, FF, dc, H.stream())
        if other is not None:
            # the weight-gradient launch (nothing but the end-of-backward fold reads it) goes to the step's OTHER stream,
            # which idles while a long tower's chain runs on this one; only dy and x have to exist, not the data gradient
            cur = torch.cuda.current_stream(x.device)
            ev = torch.cuda.Event()
            ev.record(cur)
            bwd(dx, None)
            held = (x, dy) if wsplit is None else (x, dy, wsplit, rsplit)
            StreamPlan.hand(held, other, after=ev)
            with torch.cuda.stream(other):
                bwd(None, ws)
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
                H.call("mmvae_reduce_rows", H.ptr(ws) + 4 * o, H.ptr(dst), parts, ln, rowlen, acc, H.stream())
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
    H.call("mmvae_ffn32_prep_weights_many", arr(*[w1.data_ptr() for w1, _ in pairs]), arr(*[w2.data_ptr() for _, w2 in pairs]),
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
    H.call("mmvae_gru_token_ids", H.ptr(onehot), H.ptr(ids), H.ptr(oh), B, T, V, H.stream())
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
        H.call("mmvae_gru_forward", H.ptr(pt), H.ptr(b_ih), H.ptr(w_hh), H.ptr(b_hh), H.ptr(ids), H.ptr(hs), H.ptr(saved),
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
        H.call("mmvae_gru_backward", H.ptr(dh), H.ptr(w_hh), H.ptr(hs), H.ptr(saved), H.ptr(dgx), H.ptr(dgh), T, B, Hd,
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
        H.call("mmvae_gru_cell0_fwd", H.ptr(pt), H.ptr(b_ih), H.ptr(b_hh), H.ptr(ids_last), H.ptr(h_fwd), H.ptr(out),
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
        H.call("mmvae_gru_cell0_bwd", H.ptr(dout), H.ptr(saved), H.ptr(b_hh), H.ptr(dgx), H.ptr(dgh), B, Hd, H.stream())
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
    H.call("mmvae_adam_amsgrad_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), lr, beta1, beta2,
           eps, int(step), H.ptr(step_dev), grad_scale, int(zero_grad), H.stream())


def adabelief_flat(p, g, m, s, lr, beta1, beta2, eps, step, step_dev=None, grad_scale=1.0, zero_grad=True):
    WEIGHT_GEN[0] += 1
    H.call("mmvae_adabelief_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(s), p.numel(), lr, beta1, beta2, eps, int(step),
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
    H.call("mmvae_adam_fold_flat", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), lr, beta1, beta2, eps,
           H.ptr(step_dev), grad_scale, int(zero_grad), ctypes.byref(deferred["table"]), *_tail_args(deferred["tail"]),
           H.stream())


def adam_fold_range(p, g, m, v, vmax, lo, hi, advance, lr, beta1, beta2, eps, step_dev, grad_scale, zero_grad, table, tail=None):
    """the same over elements [lo, hi) only, with the segments of `table` (H.ReduceSegments or None) that lie inside
    (mmvae_adam_fold_range); advance: this is the launch that closes the step"""
    WEIGHT_GEN[0] += 1
    H.call("mmvae_adam_fold_range", H.ptr(p), H.ptr(g), H.ptr(m), H.ptr(v), H.ptr(vmax), p.numel(), int(lo), int(hi),
           int(advance), lr, beta1, beta2, eps, H.ptr(step_dev), grad_scale, int(zero_grad),
           ctypes.byref(table) if table is not None else None, *_tail_args(tail), H.stream())


def step_inc(step_dev):
    H.call("mmvae_step_inc", H.ptr(step_dev), H.stream())


class Sigmoid(Function):
    @staticmethod
    def forward(ctx, x):
        x = H.f32c(x)
        y = torch.empty_like(x)
        H.call("mmvae_sigmoid_fwd", H.ptr(x), H.ptr(y), x.numel(), H.stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        H.call("mmvae_sigmoid_bwd", H.ptr(H.f32c(dy)), H.ptr(y), H.ptr(dx), y.numel(), H.stream())
        return dx


def sigmoid(x):
    return Sigmoid.apply(x)


def randn(shape, state):
    """standard-normal tensor from the counter-based device generator (`state`: int32[3] = seed, counter, ticket)"""
    out = torch.empty(shape, device=state.device)
    H.call("mmvae_randn", H.ptr(out), out.numel(), H.ptr(state), H.stream())
    return out


def rand_laplace(shape, state):
    """standard-Laplace variates (Laplace.rsample: z = loc + scale * e) from the counter-based device generator"""
    out = torch.empty(shape, device=state.device)
    H.call("mmvae_rand_laplace", H.ptr(out), out.numel(), H.ptr(state), H.stream())
    return out


def expand_image_u8(src_u8, dst):
    """dst (fp32, same numel) = src_u8 / 255, bit-identical to torch's true division of the converted bytes"""
    assert src_u8.dtype == torch.uint8 and dst.dtype == torch.float32 and src_u8.numel() == dst.numel()
    assert src_u8.is_contiguous() and dst.is_contiguous()
    H.call("mmvae_expand_image_u8", H.ptr(src_u8), H.ptr(dst), dst.numel(), H.stream())
    return dst


def expand_text_tokens(tokens, lengths, onehot, mask_u8=None):
    """tokens (B,T) int32 (-1 = outside the alphabet), lengths (B) int32 -> onehot (B,T,V) fp32, mask (B,T) bytes"""
    assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and onehot.dtype == torch.float32
    B, T, V = onehot.shape
    assert tokens.shape == (B, T) and lengths.shape == (B,) and tokens.is_contiguous() and onehot.is_contiguous()
    H.call("mmvae_expand_text_tokens", H.ptr(tokens), H.ptr(lengths), H.ptr(onehot), H.ptr(mask_u8), B, T, V, H.stream())
    return onehot


def fill(t, value):
    H.call("mmvae_fill", H.ptr(t), t.numel(), float(value), H.stream())


# ---- the evaluation metrics (forward only, no autograd): one module per kernel file, their public names under `ops` ------
from .metrics.loglik import *              # noqa: E402,F401,F403
from .metrics.probe import *               # noqa: E402,F401,F403
from .metrics.coherence import *           # noqa: E402,F401,F403
from .metrics.digits import *              # noqa: E402,F401,F403
from .metrics.tsne import *                # noqa: E402,F401,F403
from .metrics.frechet import *             # noqa: E402,F401,F403
from .metrics.manifold import *            # noqa: E402,F401,F403
from .metrics.kid import *                 # noqa: E402,F401,F403
from .metrics.cluster import *             # noqa: E402,F401,F403
from .metrics.gmm import *                 # noqa: E402,F401,F403
from .metrics.cca import *                 # noqa: E402,F401,F403
from .metrics.image_quality import *       # noqa: E402,F401,F403
from .metrics.text_quality import *        # noqa: E402,F401,F403
from .metrics.aggpost import *             # noqa: E402,F401,F403
from .metrics.retrieval import *           # noqa: E402,F401,F403
from .metrics.swd import *                 # noqa: E402,F401,F403
from .metrics.mmd import *                 # noqa: E402,F401,F403
