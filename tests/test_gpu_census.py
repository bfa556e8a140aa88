"""The census on the GPU: every row of every table of tests/_census.py is built, sent through the ops entry point a caller
would use (no environment knob), and has to come back (a) from the kernel instance the table names and (b) equal to the
project's reference for the operation:

    fp32 REFERENCE                   the oracle's bits (tests/_bits.py)
    FAST single-chain paths          the bits of oracle.rows_fma on the format's row list (tests/_fma_chain.py)
    FAST csr_split / csr_hybrid      the derived any-order bound; the rows of the row-gather body bitwise
    FAST bsr_mfma_f32                1e-5 * sum|a||b| (tests/test_gpu_spmm.py)
    fp64                             tests/_ref64.py bitwise in REFERENCE mode, the fp64 fma chain in FAST mode
    bf16 MFMA products               the oracle on bf16-rounded operands within the bounds of test_bsr_bf16_mfma, and a product
                                     of small integers bit for bit
    SDDMM, softmax                   tests/_sddmm_ref.py, _sddmm_bsr_ref.py, _softmax_ref.py, _softmax_bsr_ref.py and the
                                     header's bounds

Every dense result is written through a view of a larger buffer: a leading dimension above N and one row behind the last,
both full of a sentinel that has to survive.  After the rows of a family its set check compares the keys met with the table:
a key the table does not know and a key never reached both fail."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, formats, ops, synth  # noqa: E402

import _census as census  # noqa: E402
import _fma_chain as fc  # noqa: E402
import _ref64  # noqa: E402
import _sddmm_bsr_ref as sbr  # noqa: E402
import _sddmm_ref as sdr  # noqa: E402
import _softmax_bsr_ref as smb  # noqa: E402
import _softmax_ref as smr  # noqa: E402
from _bits import assert_same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = {}            # family -> {row key: key met}
TILINGS = {}         # (P, Q) -> tags of row_gather launches that passed their bitwise check

_SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.float64: (torch.int64, 0x7FF8DEAD7FC0DEAD), torch.int16: (torch.int16, 0x7FDE)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    capi.lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sentinel_out(rows, cols, pad, dtype=torch.float32):
    """(buffer [rows + 1, cols + pad] full of the sentinel, its view [:rows, :cols] for the kernel to write)."""
    as_int, bits = _SENTINEL[dtype]
    buf = torch.empty((rows + 1, cols + pad), dtype=dtype, device="cuda")
    buf.view(as_int).fill_(bits)
    return buf, buf[:rows, :cols]


def assert_sentinel(buf, rows, cols, what):
    as_int, bits = _SENTINEL[buf.dtype]
    raw = buf.view(as_int).cpu().numpy()
    gap, tail = raw[:rows, cols:], raw[rows:]
    assert np.all(gap == bits) and np.all(tail == bits), \
        f"{what}: {int((gap != bits).sum())} elements of the gap and {int((tail != bits).sum())} behind the last row were written"


def flat_out(count, dtype):
    """A 1-D or block output as the head of a longer buffer: (buffer, head of `count` leading elements / blocks)."""
    shape = (count + 3,) if isinstance(count, int) else (count[0] + 1,) + tuple(count[1:])
    as_int, bits = _SENTINEL[dtype]
    buf = torch.empty(shape, dtype=dtype, device="cuda")
    buf.view(as_int).fill_(bits)
    return buf, buf[:count if isinstance(count, int) else count[0]]


def assert_flat_sentinel(buf, count, what):
    as_int, bits = _SENTINEL[buf.dtype]
    tail = buf.view(as_int)[count:].cpu().numpy()
    assert np.all(tail == bits), f"{what}: {int((tail != bits).sum())} elements behind the output were written"


def host_f32(out):
    a = out.cpu().numpy()
    return sbr.from_bits(a) if a.dtype == np.int16 else a


# ------------------------------------------------------------------------------------------------ fp32 / fp64 SpMM of a row list
def gather_body_rows(row_ptrs, share_len):
    spans = ops.csr_spans_by_length(row_ptrs, share_len)
    return spans[ops.spans_long_count(spans):, 0].astype(np.int64)


def check_spmm(got, tag, acc, want_ref, rows, b, share_len, what):
    """got against the reference the tag's path promises."""
    if acc == "reference":
        if got.dtype == np.float64:
            _ref64.assert_same_bits64(got, _ref64.ref_rows(*rows, b), what)
        else:
            assert_same_bits(got, want_ref(), what)
        return
    from oracle import oracle as orc
    if tag.startswith(("csr_split<", "csr_hybrid<")):
        exact, bound = fc.exact_and_bound(rows, b)
        err = np.abs(got.astype(np.float64) - exact)
        worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
        print(f"{what}: worst err / any-order bound = {worst:.3f}")
        assert np.all(err <= bound), f"{what}: err / bound up to {worst:.3g}"
        if tag.startswith("csr_hybrid<"):
            chain = orc.rows_fma(*rows, b)
            short = gather_body_rows(rows[0], share_len)
            assert short.size > 0
            assert_same_bits(got[short], chain[short], f"{what}: rows of the row-gather body")
        return
    chain = orc.rows_fma(*rows, b)
    (_ref64.assert_same_bits64 if chain.dtype == np.float64 else assert_same_bits)(got, chain, what)


def run_spmm(spec, oracle, alter=None, check=True):
    """One CSR / COO / ELL product of spec; returns the tags of its launches.  alter: a hook on the result (self-test)."""
    host = census.spmm_operands(spec)
    csr, b = host["csr"], host["b"]
    fmt, acc, n, m = spec["fmt"], spec["acc"], spec["n"], csr.num_rows
    f64 = bool(spec.get("f64"))
    tdt = torch.float64 if f64 else torch.float32
    kernel = spec.get("kernel", 0)
    share_len = 0
    if fmt == "csr":
        rows = fc.csr_rows(csr, np.float64 if f64 else np.float32)
        want_ref = lambda: oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b)                     # noqa: E731
        a = ops.DeviceCSR.from_host(csr, spans=spec.get("spans"), plan=spec.get("plan"), dtype=tdt)
        if spec.get("plan"):
            assert a.plan is not None
            a.tuned[(n, acc)] = (True, (0.0, 0.0))          # the autotuner's verdict, as use_plan remembers it: take the plan
        call = lambda bd, out: ops.spmm_csr(a, bd, out=out, kernel=kernel, acc=acc)                    # noqa: E731
        batch_call = lambda bds, outs: ops.spmm_csr_batch(a, bds, outs=outs, acc=acc)                  # noqa: E731
    elif fmt == "coo":
        coo = formats.csr_to_coo(csr)
        rows = fc.coo_rows(coo)
        want_ref = lambda: oracle.spmm_coo(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data, b)       # noqa: E731
        a = ops.DeviceCOO.from_host(coo)
        if spec.get("spans") is False:                          # a COO uploaded without its span list
            a = ops.DeviceCOO(a.num_rows, a.num_cols, a.nnz, a.row_idxs, a.col_idxs, a.data)
        share_len = 0xFFFFFFFF
        call = lambda bd, out: ops.spmm_coo(a, bd, out=out, acc=acc, workspace=spec.get("workspace", True))   # noqa: E731
    else:
        assert fmt == "ell"
        ellc = formats.csr_to_ell_colmajor(csr)
        rows = fc.ell_colmajor_rows(ellc)
        want_ref = lambda: oracle.spmm_ell_colmajor(ellc.num_rows, ellc.row_idxs, ellc.data, b)        # noqa: E731
        a = ops.DeviceELL.from_host(ellc, compact=False)
        call = lambda bd, out: ops.spmm_ell(a, bd, out=out, acc=acc)                                   # noqa: E731
    pad = 2 if f64 else 4
    what = f"{fmt} {spec['rows']} N={n} {acc}"
    if spec.get("batch"):
        bs = [b] + [census.dense(csr.num_cols, n, seed=i) for i in range(1, spec["batch"])]
        outs = [sentinel_out(m, n, pad, tdt) for _ in bs]
        batch_call([dev(x) for x in bs], [o[1] for o in outs])
        tag = capi.last_kernel()
        if not check:
            return [tag]
        for i, (x, (buf, view)) in enumerate(zip(bs, outs)):
            got = view.cpu().numpy()
            if alter:
                alter(got)
            ref_i = (lambda x=x: oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, x))
            check_spmm(got, tag, acc, ref_i, rows, x, share_len, f"{what} operand {i} [{tag}]")
            assert_sentinel(buf, m, n, f"{what} operand {i} [{tag}]")
        return [tag]
    buf, view = sentinel_out(m, n, pad, tdt)
    call(dev(b), view)
    tag = capi.last_kernel()
    if not check:
        return [tag]
    got = view.cpu().numpy()
    if alter:
        alter(got)
    check_spmm(got, tag, acc, want_ref, rows, b, share_len, f"{what} [{tag}]")
    assert_sentinel(buf, m, n, f"{what} [{tag}]")
    return [tag]


def run_bsr(spec, oracle, alter=None, check=True):
    """mispmm_bsr_f32: bsr_valu, bsr_rowblock, bsr_mfma_f32."""
    host = census.bsr_operands(spec)
    bsr, b = host["bsr"], host["b"]
    n, acc, bs = spec["n"], spec["acc"], spec["bs"]
    buf, view = sentinel_out(bsr.num_rows, n, 4)
    ops.spmm_bsr(ops.DeviceBSR.from_host(bsr), dev(b), out=view, kernel=spec["kernel"], acc=acc)
    tag = capi.last_kernel()
    if not check:
        return [tag]
    got = view.cpu().numpy()
    if alter:
        alter(got)
    what = f"bsr {bs}x{bs} N={n} {acc} [{tag}]"
    want = oracle.spmm_bsr(bsr.num_rows, bs, bs, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data, b)
    if acc == "reference":
        assert_same_bits(got, want, what)
    elif tag.startswith("bsr_mfma_f32"):
        scale = np.abs(bsr.to_dense()).astype(np.float64) @ np.abs(b).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= 1e-5 * scale + 1e-37), f"{what}: max err / bound {np.max(err / (1e-5 * scale + 1e-37)):.3g}"
    else:
        assert_same_bits(got, oracle.rows_fma(*fc.bsr_rows(bsr, skip_zeros=False), b), what)
    assert_sentinel(buf, bsr.num_rows, n, what)
    return [tag]


def run_bf16(spec, oracle, alter=None, check=True):
    """The bf16 MFMA products: full-mantissa operands within the stated bound, small integers bit for bit."""
    host = census.bsr_operands(spec)
    bsr, n, out_bf16, bs = host["bsr"], spec["n"], spec["out_bf16"], spec["bs"]
    tags = []
    for kind in ("full", "ints") if check else ("full",):
        if kind == "full":
            blocks, b = synth.bf16_round(bsr.data.reshape(-1)).reshape(bsr.data.shape), synth.bf16_round(host["b"].reshape(-1)).reshape(host["b"].shape)
        else:
            rng = np.random.default_rng(17)
            blocks = np.where(bsr.data != 0, rng.integers(-4, 5, bsr.data.shape), 0).astype(np.float32)
            b = rng.integers(-8, 9, host["b"].shape).astype(np.float32)
        a16 = formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, bs, bs, bsr.block_row_ptrs, bsr.block_col_idxs, blocks)
        b_bits = dev(sbr.to_bits(b))
        buf, view = sentinel_out(bsr.num_rows, n, 8, torch.int16 if out_bf16 else torch.float32)
        if spec["op"] == "bsr":
            ops.spmm_bsr_bf16(ops.DeviceBSR.from_host(a16), dev(sbr.to_bits(blocks.reshape(-1))), b_bits, out_bf16=out_bf16, out=view)
        elif spec["op"] == "bsrc":
            ops.spmm_bsrc_bf16(ops.DeviceBSRC.from_host(a16), b_bits, out_bf16=out_bf16, out=view)
        else:
            ops.spmm_bsrc_slots_bf16(ops.DeviceBSRCSlots.from_host(a16), b_bits, out_bf16=out_bf16, out=view)
        tag = capi.last_kernel()
        tags.append(tag)
        if not check:
            continue
        got = host_f32(view)
        if alter:
            alter(got)
        what = f"{spec['op']} bf16 {bs}x{bs} N={n} {kind} [{tag}]"
        ref = oracle.spmm_bsr(bsr.num_rows, bs, bs, bsr.block_row_ptrs, bsr.block_col_idxs, blocks, b)
        if kind == "ints":
            want = synth.bf16_round(ref) if out_bf16 else ref
            assert_same_bits(got, want.astype(np.float32) + np.float32(0), what)
        else:
            scale = np.abs(a16.to_dense()).astype(np.float64) @ np.abs(b).astype(np.float64)
            lim = 2e-6 * scale + 1e-30 + (2 ** -8 * np.abs(ref) if out_bf16 else 0.0)
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= lim), f"{what}: max err / bound {np.max(err / lim):.3g}"
        assert_sentinel(buf, bsr.num_rows, n, what)
    return tags


def run_tiles(spec, oracle, alter=None, check=True):
    host = census.spmm_operands(dict(spec, fmt="csr"))
    csr, b = host["csr"], host["b"]
    return _run_csr_layout(spec, oracle, csr, b, lambda bd, out: ops.spmm_csr_tiles(ops.DeviceCSRTiles.from_host(csr), bd, out=out, acc=spec["acc"]), alter, check)


def run_panels(spec, oracle, alter=None, check=True):
    host = census.spmm_operands(dict(spec, fmt="csr"))
    csr, b = host["csr"], host["b"]
    a = ops.DeviceCSRPanels.from_host(csr, panel_rows=spec["panel_rows"])
    return _run_csr_layout(spec, oracle, csr, b, lambda bd, out: ops.spmm_csr_panels(a, bd, out=out, acc=spec["acc"]), alter, check)


def _run_csr_layout(spec, oracle, csr, b, call, alter, check):
    n, acc = spec["n"], spec["acc"]
    buf, view = sentinel_out(csr.num_rows, n, 4)
    call(dev(b), view)
    tag = capi.last_kernel()
    if not check:
        return [tag]
    got = view.cpu().numpy()
    if alter:
        alter(got)
    what = f"{spec['rows']} N={n} {acc} [{tag}]"
    check_spmm(got, tag, acc, lambda: oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), fc.csr_rows(csr), b, 0, what)
    assert_sentinel(buf, csr.num_rows, n, what)
    return [tag]


# ------------------------------------------------------------------------------------------------ SDDMM
def run_sddmm_csr(spec, oracle, alter=None, check=True):
    csr = census.spmm_operands(dict(spec, fmt="csr", n=1))["csr"]
    n, acc, f64 = spec["n"], spec["acc"], bool(spec.get("f64"))
    ndt, tdt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    tags = []
    for kind, make in (("full", sdr.full_mantissa), ("ints", sdr.small_ints))[:2 if check else 1]:
        rng = np.random.default_rng(1000 + n)
        x, y = make(rng, (csr.num_rows, n), ndt), make(rng, (csr.num_cols, n), ndt)
        buf, head = flat_out(csr.nnz, tdt)
        ops.sddmm_csr(a, dev(x), dev(y), out=head, acc=acc)
        tag = capi.last_kernel()
        tags.append(tag)
        if not check:
            continue
        exact, scale = sdr.sddmm_exact(csr.row_ptrs, csr.col_idxs, x, y)
        got = head.cpu().numpy()
        if alter:
            alter(got)
        what = f"sddmm_csr N={n} {kind} {acc} [{tag}]"
        if kind == "ints":
            assert np.array_equal(got.astype(np.float64), exact), f"{what}: {int((got != exact).sum())} entries differ"
        else:
            sdr.assert_within(got, ndt, acc, n, exact, scale, what)
        assert_flat_sentinel(buf, csr.nnz, what)
    return tags


def _pattern_device(p):
    u32 = lambda v: dev(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32))   # noqa: E731
    return ops.DeviceBSR(p.num_rows, p.num_cols, p.block_row_size, p.block_col_size, p.num_blocks, u32(p.block_row_ptrs),
                         u32(p.block_col_idxs), torch.empty(0, device="cuda"))


def run_sddmm_bsr(spec, oracle, alter=None, check=True):
    p = sbr.pattern(spec["pattern"])
    n, out_bf16, bs = spec["n"], spec["out_bf16"], p.block_row_size
    a = _pattern_device(p)
    tags = []
    for kind, make in (("wide", sbr.wide_exponent), ("ints", sbr.small_ints))[:2 if check else 1]:
        rng = np.random.default_rng(2000 + n)
        x, y = make(rng, (p.num_rows, n)), make(rng, (p.num_cols, n))
        buf, head = flat_out((p.num_blocks, bs, bs), torch.int16 if out_bf16 else torch.float32)
        ops.sddmm_bsr_bf16(a, dev(sbr.to_bits(x)), dev(sbr.to_bits(y)), out_bf16=out_bf16, out=head)
        tag = capi.last_kernel()
        tags.append(tag)
        if not check:
            continue
        exact, scale = sbr.sddmm_bsr_exact(p, x, y)
        got = host_f32(head)
        if alter:
            alter(got)
        what = f"sddmm_bsr {spec['pattern']} N={n} {kind} [{tag}]"
        if kind == "ints":
            want = synth.bf16_round(exact.astype(np.float32)) if out_bf16 else exact
            assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), f"{what}: {int((got != want).sum())} elements differ"
        else:
            sbr.assert_within(got, out_bf16, n, exact, scale, what)
        assert_flat_sentinel(buf, p.num_blocks, what)
    return tags


# ------------------------------------------------------------------------------------------------ softmax
def run_softmax_csr(spec, oracle, alter=None, check=True, bwd=False):
    g, acc, f64 = spec["g"], spec["acc"], bool(spec.get("f64"))
    ndt, tdt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    ptr = census.softmax_csr_pattern(g)
    m, nnz = ptr.shape[0] - 1, int(ptr[-1])
    a = ops.DeviceCSR(m, nnz, nnz, dev(ptr.view(np.int32)), torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=tdt, device="cuda"))
    s = smr.scores("wide", nnz, ndt, seed=g)
    length = smr.row_lengths(ptr)
    buf, head = flat_out(nnz, tdt)
    if not bwd:
        ops.softmax_csr(a, dev(s), out=head, acc=acc)
        tag = capi.last_kernel()
        if not check:
            return [tag]
        exact, t = smr.softmax_rows(ptr, s), smr.spread(ptr, s)
        got = head.cpu().numpy()
        if alter:
            alter(got)
        smr.assert_inside(got, exact, smr.fwd_bound(ndt, acc, length, t, exact), f"softmax_csr G{g} {acc} [{tag}]")
    else:
        p = smr.softmax_rows(ptr, smr.scores("narrow", nnz, ndt, seed=g)).astype(ndt)
        dp = smr.full_mantissa(np.random.default_rng(10), nnz, ndt)
        ops.softmax_csr_bwd(a, dev(p), dev(dp), out=head, acc=acc)
        tag = capi.last_kernel()
        if not check:
            return [tag]
        exact, cap = smr.softmax_bwd_rows(ptr, p, dp)
        got = head.cpu().numpy()
        if alter:
            alter(got)
        smr.assert_inside(got, exact, smr.bwd_bound(ndt, acc, length, p, dp, cap, exact), f"softmax_csr_bwd G{g} {acc} [{tag}]")
    assert_flat_sentinel(buf, nnz, tag)
    return [tag]


def run_softmax_bsr(spec, oracle, alter=None, check=True, bwd=False):
    name, out_bf16 = spec["pattern"], spec["out_bf16"]
    p = smb.pattern(name)
    bs, scale = p.block_row_size, 0.3
    a = _pattern_device(p)
    length = smb.lengths(name)
    buf, head = flat_out((p.num_blocks, bs, bs), torch.int16 if out_bf16 else torch.float32)
    if not bwd:
        s = smb.scores("wide", name)
        mask = smb.random_mask(name) if spec["mask"] else None
        ops.softmax_bsr(a, dev(s), scale=scale, mask=dev(mask) if mask is not None else None, out_bf16=out_bf16, out=head)
        tag = capi.last_kernel()
        if not check:
            return [tag]
        exact, t = smb.forward(name, smb.z_values(s, mask, scale))
        got = host_f32(head)
        if alter:
            alter(got)
        smb.assert_inside(got, exact, smb.fwd_bound(out_bf16, length, t, exact), f"softmax_bsr {name} [{tag}]")
    else:
        prob = smb.forward_f32(name, smb.z_values(smb.scores("narrow", name), None, scale))
        if spec["p_bf16"]:
            prob = smb.bf16_round(prob)
        dp = smb.full_mantissa(np.random.default_rng(10), length.shape)
        pd = dev(sbr.to_bits(prob)) if spec["p_bf16"] else dev(prob)
        ops.softmax_bsr_bwd(a, pd, dev(dp), scale=scale, out_bf16=out_bf16, out=head)
        tag = capi.last_kernel()
        if not check:
            return [tag]
        exact, cap = smb.backward(name, prob, dp, scale)
        got = host_f32(head)
        if alter:
            alter(got)
        smb.assert_inside(got, exact, smb.bwd_bound(out_bf16, length, prob, dp, cap, scale, exact), f"softmax_bsr_bwd {name} [{tag}]")
    assert_flat_sentinel(buf, p.num_blocks, tag)
    return [tag]


RUNNERS = {
    "row_gather": run_spmm, "csr_k1": run_spmm, "csr_k2": run_spmm, "csr_k3": run_spmm, "csr_wave_deep": run_spmm, "csr_split": run_spmm,
    "csr_hybrid": run_spmm, "coo_k1": run_spmm, "csr_f64": run_spmm, "bsr_valu": run_bsr, "bsr_rowblock": run_bsr, "bsr_mfma_f32": run_bsr,
    "bsr_mfma_bf16": run_bf16, "bsr_mfma_bf16_b32": run_bf16, "bsrc_mfma_bf16": run_bf16, "bsrc_slots_mfma_bf16": run_bf16,
    "csr_lds_tile": run_tiles, "csr_panel": run_panels, "sddmm_csr": run_sddmm_csr, "sddmm_bsr": run_sddmm_bsr,
    "softmax_csr": run_softmax_csr, "softmax_csr_bwd": lambda s, o, alter=None, check=True: run_softmax_csr(s, o, alter, check, bwd=True),
    "softmax_bsr": run_softmax_bsr, "softmax_bsr_bwd": lambda s, o, alter=None, check=True: run_softmax_bsr(s, o, alter, check, bwd=True),
}


def run_row(family, row, oracle, alter=None):
    """Run one table row: every launch it makes must come from the row's instance; the key met is recorded first, so that
    the family's set check can name an instance the table does not know."""
    tags = RUNNERS[family](row.spec, oracle, alter, True)
    keys = {census.normalise(t) for t in tags}
    SEEN.setdefault(family, {})[row.key] = sorted(keys)[0] if len(keys) == 1 else " | ".join(sorted(keys))
    assert keys == {row.key}, f"{family}: the table expects {row.key!r}, the library ran {sorted(keys)} ({tags})"
    if family == "row_gather" and row.spec["acc"] == "reference":
        for t in tags:
            TILINGS.setdefault(census.xcd_of(t), []).append(t)
    return tags


_SWEPT = {}          # id of a sweep's spec list -> the keys it met (families that share a sweep run it once)


def sweep(family, oracle):
    """Launch the family's sweep (census.SWEEPS) without comparing anything and return the keys met.  A shape an entry point
    declines is not a launch."""
    specs = census.SWEEPS[family]
    if id(specs) not in _SWEPT:
        met = {}
        for spec in specs:
            try:
                tags = RUNNERS[family](spec, oracle, None, False)
            except (capi.MispmmError, ValueError):
                continue
            for t in tags:
                met.setdefault(census.normalise(t), spec)
        torch.cuda.synchronize()
        _SWEPT[id(specs)] = met
    return _SWEPT[id(specs)]


def set_check(family, oracle):
    """The keys met equal the table's keys.  Rows that have not run in this session (the test was selected alone) run here;
    then the family's sweep, every key of which -- of this family or of another -- has to be a row of its table."""
    rows = census.FAMILIES[family]
    met = SEEN.setdefault(family, {})
    for row in rows:
        if row.key not in met:
            try:
                run_row(family, row, oracle)
            except AssertionError as e:          # the comparison's failure belongs to the row's own item; the key is recorded
                print(f"{family} {row.key}: {e}")
    swept = sweep(family, oracle)
    known = {f: {r.key for r in rs} for f, rs in census.FAMILIES.items()}
    strangers = {k: spec for k, spec in swept.items() if k not in known.get(census.family_of(k), ())}
    table = known[family]
    seen = set(met.values()) | {k for k in swept if census.family_of(k) == family}
    unknown, missing = sorted(seen - table), sorted(table - seen)
    print(f"{family}: {len(seen & table)} of {len(table)} keys of the table met; the sweep of {len(census.SWEEPS[family])} launches met {len(swept)} keys")
    assert not strangers, f"{family}: the sweep met instances no table knows: {strangers}"
    assert not unknown, f"{family}: instances the table must learn: {unknown}"
    assert not missing, f"{family}: instances never reached: {missing}"


def _make_tests(family):
    rows = census.FAMILIES[family]

    @pytest.mark.parametrize("row", rows, ids=[r.key for r in rows])
    def test_rows(row, oracle):
        run_row(family, row, oracle)

    def test_set(oracle):
        set_check(family, oracle)

    test_rows.__name__ = test_rows.__qualname__ = f"test_{family}_instances"
    test_set.__name__ = test_set.__qualname__ = f"test_{family}_set_of_keys"
    return test_rows, test_set


for _family in census.FAMILIES:
    if census.FAMILIES[_family]:
        globals()[f"test_{_family}_instances"], globals()[f"test_{_family}_set_of_keys"] = _make_tests(_family)


def test_row_gather_runs_all_four_xcd_tilings(oracle):
    """8x1, 4x2, 2x4 and 1x8: every tiling xcd_tiling can return, each with the bitwise check of REFERENCE mode."""
    for (p, q), spec in census.ROW_GATHER_TILINGS.items():
        tags = run_spmm(spec, oracle)
        assert [census.xcd_of(t) for t in tags] == [(p, q)] and tags[0].startswith("row_gather<"), f"N={spec['n']}: expected xcd {p}x{q}, ran {tags}"
        TILINGS.setdefault((p, q), []).extend(tags)
    print("row_gather tilings met:", {f"{p}x{q}": len(v) for (p, q), v in sorted(TILINGS.items())})
    assert set(TILINGS) == {(8, 1), (4, 2), (2, 4), (1, 8)}, sorted(TILINGS)
