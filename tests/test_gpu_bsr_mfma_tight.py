"""The four checks of tests/_bsr_mfma_tight.py (the derived bound, the exact family with its bf16 ties, the special values, the
untouched elements) on the bf16 block-sparse MFMA kernels themselves, through ops.spmm_bsr_bf16, ops.spmm_bsrc_bf16 and
ops.spmm_bsrc_slots_bf16, for an fp32 and a bf16 C, on the cases tests/test_bsr_mfma_mutants_cpu.py mutation-checks.  The oracle
is not the reference here (numpy in np.longdouble is); one test holds the oracle to the same tolerance.  The two knob-only
instances (bsr_bf16_lds, `share` with a bf16 C) are not run here: tests/test_gpu_spmm.py reaches them in child processes."""
import numpy as np
import pytest
import torch

import _bsr_mfma_mutants as mut
import _bsr_mfma_tight as tight
import _sddmm_bsr_ref as sbr
from mispmm import capi, ops

pytestmark = pytest.mark.gpu


def expected_tag(case):
    c = "c16" if case.out_bf16 else "c32"
    if case.kernel in ("bsr16", "bsr32"):
        t = 8 if case.n >= 128 and case.n % 8 == 0 and case.ldb % 8 == 0 and case.ldc % 8 == 0 else 4
        return f"bsr_mfma_bf16{'_b32' if case.kernel == 'bsr32' else ''}<T{t},{c}>"
    if case.kernel == "bsrc":
        return f"bsrc_mfma_bf16<{c}>"
    return f"bsrc_slots_mfma_bf16<{c},nt{',share' if mut.shares(case, tight.operands(case)['bsr']) else ''}>"


_UPLOADS = {}


def _upload(kernel, bsr, key):
    if (kernel, key) not in _UPLOADS:
        make = {"bsr16": ops.DeviceBSR, "bsr32": ops.DeviceBSR, "bsrc": ops.DeviceBSRC, "slots": ops.DeviceBSRCSlots}[kernel]
        _UPLOADS[kernel, key] = make.from_host(bsr)
    return _UPLOADS[kernel, key]


def run(case):
    """The kernel's flat C buffer, as tight.c_view takes it."""
    host = tight.operands(case)
    bsr = host["bsr"]
    m, k = bsr.num_rows, bsr.num_cols
    bbuf = torch.from_numpy(sbr.to_bits(np.full((k, case.ldb), 3.0, np.float32))).cuda()
    bbuf[:, :case.n] = torch.from_numpy(_bits(host["b"])).cuda()
    sentinel = tight.SENTINEL
    if case.out_bf16:
        cbuf = torch.from_numpy(sbr.to_bits(np.full(m * case.ldc + tight.TAIL, sentinel, np.float32))).cuda()
    else:
        cbuf = torch.full((m * case.ldc + tight.TAIL,), float(sentinel), dtype=torch.float32, device="cuda")
    out = cbuf[:m * case.ldc].view(m, case.ldc)[:, :case.n]
    a = _upload(case.kernel, bsr, (case.pattern, case.kind, case.n))
    if case.kernel in ("bsr16", "bsr32"):
        blocks = torch.from_numpy(_bits(np.asarray(bsr.data, np.float32).reshape(-1))).cuda()
        ops.spmm_bsr_bf16(a, blocks, bbuf[:, :case.n], out_bf16=case.out_bf16, out=out)
    elif case.kernel == "bsrc":
        ops.spmm_bsrc_bf16(a, bbuf[:, :case.n], out_bf16=case.out_bf16, out=out)
    else:
        ops.spmm_bsrc_slots_bf16(a, bbuf[:, :case.n], out_bf16=case.out_bf16, out=out)
    assert capi.last_kernel() == expected_tag(case), (capi.last_kernel(), expected_tag(case))
    got = cbuf.cpu().numpy()
    return sbr.from_bits(got) if case.out_bf16 else got


def _bits(v):
    """float32 array of bf16 numbers, NaN and Inf among them -> int16 bf16 bits."""
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16)


def _all(check, kernel):
    worst, failed = {}, []
    for case in mut.cases_of(check, kernel):
        ok, ratio = mut.CHECKS[check](run(case), case)
        key = "bf16 C" if case.out_bf16 else "fp32 C"
        worst[key] = max(worst.get(key, 0.0), ratio)
        print(f"{check} {tight.case_id(case)} [{capi.last_kernel()}]: {'ok' if ok else 'FAILS'} {ratio:.3g}")
        if not ok:
            failed.append(tight.case_id(case))
    print(f"{kernel} {check}: worst " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not failed, failed


@pytest.mark.parametrize("kernel", mut.ALL)
def test_within_the_derived_bound(kernel):
    """|C - exact| <= g_n S (fp32 C), C between the roundings of the interval's ends (bf16 C); worst |err| / tol printed."""
    _all("tight", kernel)


@pytest.mark.parametrize("kernel", mut.ALL)
def test_exact_sums_bit_for_bit_and_their_bf16_ties(kernel):
    _all("sharp_exact", kernel)


@pytest.mark.parametrize("kernel", mut.ALL)
def test_nan_and_inf_land_where_the_contract_says(kernel):
    """0 * b is formed for every stored element by the dense-block kernels, for the occupied columns by the compacted ones, and
    for no padding slot, missing pair half or B row past a block row's end."""
    _all("specials", kernel)


@pytest.mark.parametrize("kernel", mut.ALL)
def test_empty_block_rows_are_zero_and_the_gap_and_tail_keep_their_sentinel(kernel):
    _all("untouched", kernel)


def test_the_oracle_is_inside_the_same_tolerance(oracle):
    """The fp32 CPU sum the older tests compare with rounds too; on these cases it has to sit inside the derived bound of the
    element's additions in ITS order: one per non-zero product."""
    for kernel in mut.ALL:
        case = mut.new_cases(kernel, "tight")[2 if kernel in mut.DENSE else 0]
        bsr, b = tight.operands(case)["bsr"], tight.operands(case)["b"]
        ref = oracle.spmm_bsr(bsr.num_rows, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs, bsr.block_col_idxs,
                              np.asarray(bsr.data, np.float32), b)
        flat = np.full(bsr.num_rows * case.ldc + tight.TAIL, tight.SENTINEL, np.float32)
        tight.c_view(flat, case)[:, :case.n] = ref
        ok, ratio = tight.within(flat, case._replace(out_bf16=False))
        print(f"oracle {tight.case_id(case)}: worst |err| / tol {ratio.max():.3g}")
        assert ok.all()
