"""The float32 fronts of the fused attention on a CSR pattern (ops.attention_csr, ops.attention_csr_bwd) stand on the one front of
the family (mispmm/_attn_csr.py), as the bf16 ones and the bias gradient do: the refusal tables that test_attn_csr_bf16_cpu.py
and test_attn_csr_bf16_bwd_cpu.py run against the bf16 functions are run here against the float32 ones with float32 operands.
Every row must be refused with a ValueError that names the operand and the defect, with the same substrings ("a float32 tensor"
where the bf16 table says "an int16 tensor of bf16 bits"), before any library is reached.  No GPU: the device check is replaced
by a no-op, as test_ops_contract_cpu.py does, and the side libraries' lib() by a stand-in that fails the test if reached.
Without the patch the precedence is what it was: the two ops functions say `no CPU path` first, the three side modules name the
defect first."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import attn_csr_bf16, attn_csr_dbias, capi_attn_csr, capi_attn_csr_bwd, capi_attn_csr_dbias, ops  # noqa: E402

import _attn_csr_bf16_bwd_ref as bb  # noqa: E402
from _softmax_ref import matrix  # noqa: E402

CSR = matrix("long")
M, KK, NNZ = CSR.num_rows, CSR.num_cols, CSR.nnz
f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)            # noqa: E731
bits = lambda *shape: torch.zeros(shape, dtype=torch.int16)             # noqa: E731


@pytest.fixture
def only_the_checks(monkeypatch):
    def reached():
        pytest.fail("a defective call reached a library")
    monkeypatch.setattr(ops, "_require_gpu", lambda *tensors: None)
    for side in (capi_attn_csr, capi_attn_csr_bwd, capi_attn_csr_dbias):
        monkeypatch.setattr(side, "lib", reached)


def _reversed(rows, width):
    """What a flipped view of another library looks like: a negative row stride, which no torch view has."""
    class Reversed:
        dtype, shape, is_cuda = torch.float32, (rows, width), False

        def dim(self):
            return 2

        def unsqueeze(self, _):
            return Reversed3()

        def stride(self, i=None):
            s = (-width, 1)
            return s if i is None else s[i]

    class Reversed3(Reversed):
        shape = (1, rows, width)

        def dim(self):
            return 3

        def stride(self, i=None):
            s = (0, -width, 1)
            return s if i is None else s[i]
    return Reversed()


def test_the_forward_refuses_every_defect_of_the_bf16_table(only_the_checks):
    a = ops.DeviceCSR.from_host(CSR, device="cpu")
    q, k, v = f32(M, 8), f32(KK, 8), f32(KK, 16)

    def refused(match, **kw):
        args = dict(q=q, k=k, v=v)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.attention_csr(a, args.pop("q"), args.pop("k"), args.pop("v"), **args)

    # wrong dtype
    refused("q must be a float32 tensor", q=bits(M, 8))
    refused("k must be a float32 tensor", k=torch.zeros((KK, 8), dtype=torch.bfloat16))
    refused("v must be a float32 tensor", v=torch.zeros((KK, 16), dtype=torch.float64))
    refused("bias must be a float32", bias=torch.zeros(NNZ, dtype=torch.float64))
    refused("lse must be a contiguous float32", lse=torch.zeros(M, dtype=torch.float64))
    refused("out must be a float32 tensor", out=bits(M, 16))
    # wrong rank
    refused("q must be", q=f32(M * 8))
    refused("q, k and v must all be 2-D", k=f32(1, KK, 8))
    refused("v must be", v=f32(1, 1, KK, 16))
    # wrong shape against a
    refused("q must be", q=f32(M + 1, 8))
    refused("k must be", k=f32(KK - 1, 8))
    refused("v must be", q=f32(2, M, 8), k=f32(2, KK, 8), v=f32(3, KK, 16))
    refused("same number of columns", k=f32(KK, 16))
    refused("widths from 1 to 256: v", v=f32(KK, 264))
    refused("bias must have shape", bias=torch.zeros(NNZ + 1))
    refused("bias must have shape", bias=torch.zeros((2, NNZ)))
    refused("out must be a float32 tensor of shape", out=f32(M, 8))
    refused("lse must be a contiguous float32", lse=torch.zeros(M + 1))
    # column stride != 1
    refused("q must have unit column stride", q=f32(M, 16)[:, ::2])
    refused("v must have unit column stride", v=f32(16, KK).t())
    refused("bias must have unit stride", bias=torch.zeros(2 * NNZ)[::2])
    refused("out must have unit column stride", out=f32(M, 32)[:, ::2])
    # rows that overlap
    refused("k must not overlap its own rows", k=f32(1, 8).expand(KK, 8))
    refused("out must have unit column stride and rows", out=f32(1, 16).expand(M, 16))
    # a negative stride, of an operand and (refused since the fronts are one) of out
    refused("k must not have a negative stride", k=_reversed(KK, 8))
    refused("out must have unit column stride and rows", out=_reversed(M, 16))
    # a non-contiguous lse
    refused("lse must be a contiguous float32", lse=torch.zeros((M, 2))[:, 0])
    # a float64 matrix
    with pytest.raises(ValueError, match="float32 DeviceCSR"):
        ops.attention_csr(ops.DeviceCSR.from_host(CSR, device="cpu", dtype=torch.float64), q, k, v)


def test_the_backward_refuses_every_defect_of_the_bf16_table(only_the_checks):
    t_csr, perm_np = bb.bref.transpose(CSR)
    a = ops.DeviceCSR.from_host(CSR, device="cpu")
    at = ops.DeviceCSR.from_host(t_csr, device="cpu")
    perm = torch.from_numpy(perm_np.astype(np.int32))
    good = dict(q=f32(M, 8), k=f32(KK, 8), v=f32(KK, 16), out=f32(M, 16), lse=f32(M), grad_out=f32(M, 16))

    def refused(match, at_=at, perm_=perm, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.attention_csr_bwd(a, at_, perm_, *(args.pop(n) for n in ("q", "k", "v", "out", "lse", "grad_out")), **args)

    # wrong dtype
    refused("q must be a float32 tensor", q=bits(M, 8))
    refused("k must be a float32 tensor", k=torch.zeros((KK, 8), dtype=torch.bfloat16))
    refused("v must be a float32 tensor", v=torch.zeros((KK, 16), dtype=torch.float64))
    refused("grad_out must be a float32 tensor", grad_out=bits(M, 16))
    refused("out must be a float32 tensor", out=bits(M, 16))
    refused("bias must be a float32", bias=torch.zeros(NNZ, dtype=torch.float64))
    refused("lse must be a contiguous float32", lse=torch.zeros(M, dtype=torch.float64))
    refused("delta must be a contiguous float32", delta=torch.zeros(M, dtype=torch.float64))
    refused("perm must hold", perm_=torch.zeros(NNZ))
    # a dq= / dk= / dv= of the wrong dtype
    refused("dq must be a float32 tensor", dq=bits(M, 8))
    refused("dk must be a float32 tensor", dk=torch.zeros((KK, 8), dtype=torch.bfloat16))
    refused("dv must be a float32 tensor", dv=bits(KK, 16))
    # wrong rank
    refused("q must be", q=f32(M * 8))
    refused("must all be 2-D or all", k=f32(1, KK, 8))
    refused("must all be 2-D or all", grad_out=f32(1, M, 16))
    refused("v must be", v=f32(1, 1, KK, 16))
    # wrong shape
    refused("q must be", q=f32(M + 1, 8))
    refused("k must be", k=f32(KK - 1, 8))
    refused("same number of columns", k=f32(KK, 16))
    refused("widths from 1 to 256: v", v=f32(KK, 264))
    refused("out must have shape", out=f32(M, 8))
    refused("grad_out must have shape", grad_out=f32(M + 1, 16))
    refused("dq must have shape", dq=f32(M, 16))
    refused("dv must have shape", dv=f32(M, 16))
    refused("bias must have shape", bias=torch.zeros(NNZ + 1))
    refused("lse must be a contiguous float32", lse=torch.zeros(M + 1))
    refused("delta must be a contiguous float32", delta=torch.zeros(M + 1))
    refused("perm must hold", perm_=perm[:-1])
    refused("A\\^T", at_=a)
    refused("three flags", need=(True, True))
    # column stride != 1
    refused("q must have unit column stride", q=f32(M, 16)[:, ::2])
    refused("grad_out must have unit column stride", grad_out=f32(M, 32)[:, ::2])
    refused("out must have unit column stride", out=f32(M, 32)[:, ::2])
    refused("dk must have unit column stride", dk=f32(KK, 16)[:, ::2])
    refused("bias must have unit stride", bias=torch.zeros(2 * NNZ)[::2])
    # rows that overlap
    refused("k must not overlap its own rows", k=f32(1, 8).expand(KK, 8))
    refused("grad_out must not overlap its own rows", grad_out=f32(1, 16).expand(M, 16))
    refused("dv must not overlap its own rows", dv=f32(1, 16).expand(KK, 16))
    # a negative stride
    refused("grad_out must not have a negative stride", grad_out=_reversed(M, 16))
    # a non-contiguous lse or delta
    refused("lse must be a contiguous float32", lse=torch.zeros((M, 2))[:, 0])
    refused("delta must be a contiguous float32", delta=torch.zeros((M, 2))[:, 0])
    # a missing perm with a bias where dk or dv is needed
    refused("with a bias, dk and dv need perm", perm_=None, bias=torch.zeros(NNZ))
    # a float64 matrix
    with pytest.raises(ValueError, match="float32 DeviceCSR"):
        ops.attention_csr_bwd(ops.DeviceCSR.from_host(CSR, device="cpu", dtype=torch.float64), at, perm, *good.values())


def test_without_the_patch_the_ops_functions_say_no_cpu_path_first_and_the_side_modules_name_the_defect_first():
    t_csr, perm_np = bb.bref.transpose(CSR)
    a = ops.DeviceCSR.from_host(CSR, device="cpu")
    at = ops.DeviceCSR.from_host(t_csr, device="cpu")
    perm = torch.from_numpy(perm_np.astype(np.int32))
    bad = f32(M, 16)[:, ::2]                                            # q with a column stride of 2
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_csr(a, bad, f32(KK, 8), f32(KK, 16))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_csr_bwd(a, at, perm, bad, f32(KK, 8), f32(KK, 16), f32(M, 16), f32(M), f32(M, 16))
    bad16 = bits(M, 16)[:, ::2]
    with pytest.raises(ValueError, match="q must have unit column stride"):
        attn_csr_bf16.attention_csr_bf16(a, bad16, bits(KK, 8), bits(KK, 16))
    with pytest.raises(ValueError, match="q must have unit column stride"):
        attn_csr_bf16.attention_csr_bf16_bwd(a, at, perm, bad16, bits(KK, 8), bits(KK, 16), f32(M, 16), f32(M), bits(M, 16))
    with pytest.raises(ValueError, match="q must have unit column stride"):
        attn_csr_dbias.attention_csr_dbias(a, bad, f32(KK, 8), f32(KK, 16), f32(M, 16), f32(M), f32(M, 16))
    with pytest.raises(ValueError, match="q must have unit column stride"):
        attn_csr_dbias.attention_csr_dbias_bf16(a, bad16, bits(KK, 8), bits(KK, 16), f32(M, 16), f32(M), bits(M, 16))
