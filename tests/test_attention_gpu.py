"""The attention kernels of csrc/text.hip (mmvae_attn_fwd / mmvae_attn_bwd: every instantiation a supported call can reach)
against the float64 restatement of tests/attention_reference.py, part by part: out, the saved probabilities (magnitude and
sign bit), dq, dk, dv each on its own maximum, with the tolerances tests/test_attention_reference_host.py derives.

The C ABI is called directly with separate q, k, v, dout, dq, dk, dv, each a view into an arena of its own: inputs lie in
NaN (rows past L / S, the columns between E and the leading dimension, the guards in front and behind), so a read out of
range that enters the arithmetic shows; outputs are written into a sentinel, and every element outside the logical region
must still hold it afterwards.  Behind its logical region every arena goes on to what 128 rows (probs: a 128 x 128 tile)
would take, plus a guard, so the test stays inside its own allocations whatever a kernel does with an index inside its
tiles."""
import zlib

import pytest
import torch

import attention_reference as AR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -12345.5
GUARD = 1024            # floats in front of every logical region and behind its tail (a multiple of 4: keeps 16-byte alignment)
TILE = 128              # rows / keys of the kernels' widest tile
WORST = {}              # "<kernel>:<part>" -> worst error over the module, printed at the end


@pytest.fixture(scope="module")
def ops(hip_lib):
    from multimodal_vae_comparison_amd import ops
    yield ops
    if WORST:
        print("\nworst error per kernel and part (of the part's float64 maximum):")
        for k in sorted(WORST):
            print(f"  {k}: {WORST[k]:.3e}")


@pytest.fixture(scope="module")
def H(hip_lib):
    from multimodal_vae_comparison_amd import hipops
    return hipops


class Arena:
    """rows x N x width floats with leading dimension ld, `off` floats past a 16-byte boundary, between a guard and a tail
    of `tail` floats (default: the rows up to 128) + a guard, all of them `fill`"""

    def __init__(self, rows, N, width, ld, off, fill, tail=None):
        assert ld >= width and GUARD % 4 == 0
        self.rows, self.N, self.width, self.ld, self.off = rows, N, width, ld, off
        tail = max(TILE - rows, 0) * N * ld if tail is None else tail
        self.flat = torch.full((GUARD + off + rows * N * ld + tail + GUARD,), fill, dtype=torch.float32, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.fill = fill

    def cols(self, c0, E):
        """(rows, N, E) view of columns [c0, c0 + E)"""
        assert c0 + E <= self.width
        return self.flat.as_strided((self.rows, self.N, E), (self.N * self.ld, self.ld, 1), GUARD + self.off + c0)

    def all(self):
        return self.cols(0, self.width)

    def untouched(self):
        """every element outside the logical region still holds the fill value"""
        inside = torch.zeros_like(self.flat, dtype=torch.bool)
        inside.as_strided((self.rows * self.N, self.width), (self.ld, 1), GUARD + self.off).fill_(True)
        return int((self.flat[~inside] != self.fill).sum())


def _drop(ops, c):
    """the case's own dropout state (seeded by its name) -> (spec or None, multiplier (N, H, L, S) on the CPU or None)"""
    if c.p == 0:
        return None, None
    state = torch.zeros(2 + 16, dtype=torch.int32)
    state[0] = zlib.crc32(c.name.encode()) & 0x7FFFFFFF
    state = state.to(DEV)
    ops.dropout_advance(state, 0)
    drop = ops.DropSpec(state, 0, 1, c.p, "attn")
    n = c.N * c.H * c.L * c.S
    return drop, ops.dropout_mask(drop, n).cpu().view(c.N, c.H, c.L, c.S)


def _inputs(c, inp):
    ldq, ldk, ldv, off, _ = c.geometry()
    if c.layout == "packed":
        a = Arena(c.L, c.N, 3 * c.E, 3 * c.E, 0, float("nan"))
        views = [a.cols(i * c.E, c.E) for i in range(3)]
    else:
        views = [Arena(r, c.N, c.E, ld, off, float("nan")).all() for r, ld in ((c.L, ldq), (c.S, ldk), (c.S, ldv))]
    for t, name in zip(views, "qkv"):
        t.copy_(inp[name])
    dout = Arena(c.L, c.N, c.E, c.E, 0, float("nan")).all()
    dout.copy_(inp["dout"])
    mask = None
    if inp["mask"] is not None:          # the (N, S) bytes inside bytes that would all count as set
        buf = torch.full((GUARD + c.N * c.S + TILE + GUARD,), 77, dtype=torch.uint8, device=DEV)
        mask = buf[GUARD:GUARD + c.N * c.S].view(c.N, c.S)
        mask.copy_(inp["mask"])
    return views, dout, mask


def _grad_arenas(c):
    ldq, ldk, ldv, off, _ = c.geometry()
    if c.layout == "packed":
        a = Arena(c.L, c.N, 3 * c.E, 3 * c.E, 0, SENT)
        return [a], [a.cols(i * c.E, c.E) for i in range(3)]
    arenas = [Arena(r, c.N, c.E, ld, off, SENT) for r, ld in ((c.L, ldq), (c.S, ldk), (c.S, ldv))]
    return arenas, [a.all() for a in arenas]


def _al16(*ts):
    return int(all(t.data_ptr() % 16 == 0 for t in ts))


def run_direct(c, inp, drop, lib, H, parts=None):
    """forward, then the backward from the kernel's own saved probabilities in both forms -> out, probs, {form: (dq, dk,
    dv)}; with `parts`: the sentinel and dispatch conditions are recorded there"""
    ldq, ldk, ldv, _, poff = c.geometry()
    (q, k, v), dout, mask = _inputs(c, inp)
    out_a = Arena(c.L, c.N, c.E, c.E, 0, SENT)
    probs_a = Arena(1, 1, c.N * c.H * c.L * c.S, c.N * c.H * c.L * c.S, poff, SENT, tail=TILE * TILE)
    out, probs = out_a.all(), probs_a.all().view(c.N, c.H, c.L, c.S)
    dp = drop.c() if drop is not None else None
    path = lib.mmvae_attn_path(0, c.L, c.S, c.hd, ldq, ldk, ldv, _al16(q, k, v))
    rc = lib.mmvae_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), H.ptr(mask), out.data_ptr(), probs.data_ptr(), c.L, c.S,
                            c.N, c.H, c.hd, ldq, ldk, ldv, int(c.valid), dp, H.stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{c}: mmvae_attn_fwd returned {rc}"
    if parts is not None:
        parts.require("forward kernel", path == AR.PATH_VALUE[c.fwd], f"selector gives {path}, the case names {c.fwd}")
        parts.require("out: nothing written outside (L, N, E)", out_a.untouched() == 0)
        parts.require("probs: nothing written outside (N, H, L, S)", probs_a.untouched() == 0)
    grads = {}
    was = lib.mmvae_attn_t_bwd_set(0)
    try:
        for form in (0, 1):
            lib.mmvae_attn_t_bwd_set(form)
            arenas, (dq, dk, dv) = _grad_arenas(c)
            path = lib.mmvae_attn_path(1, c.L, c.S, c.hd, ldq, ldk, ldv, _al16(q, k, v, dq, dk, dv, dout))
            rc = lib.mmvae_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), probs.data_ptr(), dout.data_ptr(), dq.data_ptr(),
                                    dk.data_ptr(), dv.data_ptr(), c.L, c.S, c.N, c.H, c.hd, ldq, ldk, ldv, dp, H.stream())
            torch.cuda.synchronize()
            assert rc == 0, f"{c}: mmvae_attn_bwd returned {rc}"
            if parts is not None:
                parts.require(f"backward kernel (form {form})", path == AR.PATH_VALUE[c.bwd[form]],
                              f"selector gives {path}, the case names {c.bwd[form]}")
                parts.require(f"gradients (form {form}): nothing written outside their regions",
                              sum(a.untouched() for a in arenas) == 0)
            grads[form] = tuple(t.clone() for t in (dq, dk, dv))
    finally:
        lib.mmvae_attn_t_bwd_set(was)
    return out.clone(), probs.clone(), grads


def _non_finite(parts, c, what, tensors):
    """the sample without a valid key: 0 / 0 throughout, as the kernels' comments promise and torch gives"""
    if c.mask != "full_sample":
        return
    for part, t in tensors:
        bad = AR.by_sample(part, t, [AR.FULLY_MASKED])
        parts.require(f"{what}{part} of the fully masked sample is non-finite", not bool(torch.isfinite(bad).any()))


@pytest.mark.parametrize("c", AR.CASES, ids=repr)
def test_attention_kernels_part_by_part(ops, H, hip_lib, c):
    inp = AR.make_inputs(c)
    drop, mult = _drop(ops, c)
    ref = AR.run_reference(c, inp, AR.F64, mult=mult)
    parts = AR.Parts(c.name, WORST)
    out, probs, grads = run_direct(c, inp, drop, hip_lib, H, parts)
    out, probs = out.cpu(), probs.cpu()
    AR.check_forward(parts, c, out, probs.abs(), ref, prefix=c.fwd + ":")
    AR.check_signs(parts, c, probs, mult)
    _non_finite(parts, c, "", (("out", out), ("probs", probs)))
    for form in (0, 1):
        dq, dk, dv = (t.cpu() for t in grads[form])
        AR.check_backward(parts, c, dq, dk, dv, ref, prefix=c.bwd[form] + ":")
        _non_finite(parts, c, f"form {form}: ", (("dq", dq), ("dk", dk), ("dv", dv)))
    parts.done()


@pytest.mark.parametrize("c", [c for c in AR.CASES if c.expressible], ids=repr)
def test_ops_attention_is_the_direct_call(ops, H, hip_lib, c):
    """the path the models take (ops.attention on a packed buffer) gives, bit for bit, what the direct C-ABI call gives"""
    inp = AR.make_inputs(c)
    drop, _ = _drop(ops, c)
    out, _, grads = run_direct(c, inp, drop, hip_lib, H)
    was = hip_lib.mmvae_attn_t_bwd_set(0)
    try:
        for form in (0, 1):
            hip_lib.mmvae_attn_t_bwd_set(form)
            qkv = torch.cat([inp["q"], inp["k"], inp["v"]], -1).to(DEV).requires_grad_(True)
            o = ops.attention(qkv, None if inp["mask"] is None else inp["mask"].to(DEV), c.H, mask_is_valid=c.valid, drop=drop)
            o.backward(inp["dout"].to(DEV))
            assert torch.equal(o.detach(), out), f"{c}: out differs"
            assert torch.equal(qkv.grad, torch.cat(grads[form], -1)), f"{c}: dqkv differs (backward form {form})"
    finally:
        hip_lib.mmvae_attn_t_bwd_set(was)


@pytest.mark.parametrize("L,S,hd", AR.LIMIT_CASES)
def test_limits_are_refused_and_write_nothing(H, hip_lib, L, S, hd):
    N, nh = 2, 1
    E = nh * hd
    q = torch.randn(L, N, E, device=DEV)
    k, v = torch.randn(S, N, E, device=DEV), torch.randn(S, N, E, device=DEV)
    dout = torch.randn(L, N, E, device=DEV)
    out, probs = torch.full((L, N, E), SENT, device=DEV), torch.full((N, nh, L, S), SENT, device=DEV)
    dq, dk, dv = (torch.full(t.shape, SENT, device=DEV) for t in (q, k, v))
    rf = hip_lib.mmvae_attn_fwd(H.ptr(q), H.ptr(k), H.ptr(v), None, H.ptr(out), H.ptr(probs), L, S, N, nh, hd, E, E, E, 0, None,
                                H.stream())
    rb = hip_lib.mmvae_attn_bwd(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(probs), H.ptr(dout), H.ptr(dq), H.ptr(dk), H.ptr(dv), L, S,
                                N, nh, hd, E, E, E, None, H.stream())
    torch.cuda.synchronize()
    assert (rf, rb) == (AR.ERR_UNSUPPORTED, AR.ERR_UNSUPPORTED)
    for name, t in (("out", out), ("probs", probs), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool((t == SENT).all()), f"{name} was written by a refused call"
