"""The census tables themselves (tests/_census.py), without a GPU: the key normaliser on one tag of every family, the tables'
form, the builders' index ranges, and the number of instances of every kernel template in the built library."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mispmm import capi

import _census as census

EXAMPLES = [     # one capi.last_kernel() string per note_kernel call site, as the launchers format them -> its key
    ("row_gather<G16,V4,ref64,uniform,B128,U8,line,S14> xcd 4x2", "row_gather<G16,V4,ref64,uniform,B128,U8,line,S14>"),
    ("row_gather<G8,V4,fast,csr,B128,U8,roll,S16> xcd 8x1 batched plan-order", "row_gather<G8,V4,fast,csr,B128,U8,roll,S16> batched plan-order"),
    ("row_gather<G32,V2,ref32,ell,B128,U8,batch,S16> xcd 8x1", "row_gather<G32,V2,ref32,ell,B128,U8,batch,S16>"),
    ("row_stream<G16,ref64,uniform,W14> xcd 4x2, 96 workgroups per XCD x 1 plan-order", "row_stream<G16,ref64,uniform,W14> plan-order"),
    ("csr_k1<G8,V4,ref64>", "csr_k1<G8,V4,ref64>"),
    ("csr_k2<G64,V1,fast>", "csr_k2<G64,V1,fast>"),
    ("csr_wide<G16,V2,fast>", "csr_wide<G16,V2,fast>"),
    ("csr_k3<V2,R2,ref64>", "csr_k3<V2,R2,ref64>"),
    ("csr_wave_deep<V1,fast>", "csr_wave_deep<V1,fast>"),
    ("csr_split<W4,R8,ref64,longest-first> xcd 2x4", "csr_split<W4,R8,ref64,longest-first>"),
    ("csr_hybrid<fast,R8> split 8 spans xcd 4x2 + row_gather<G8,spans> 92 rows xcd 4x2 aligned", "csr_hybrid<fast,R8>+row_gather<G8,spans>"),
    ("coo_k1<G8,V4,ref32,wide>", "coo_k1<G8,V4,ref32,wide>"),
    ("bsr_valu<G16,V4,ref32>", "bsr_valu<G16,V4,ref32>"),
    ("bsr_rowblock<BD16,RS8,V2,fast>", "bsr_rowblock<BD16,RS8,V2,fast>"),
    ("bsr_mfma_f32", "bsr_mfma_f32"),
    ("bsr_mfma_bf16<T8,c16>", "bsr_mfma_bf16<T8,c16>"),
    ("bsr_mfma_bf16_b32<T4,c32>", "bsr_mfma_bf16_b32<T4,c32>"),
    ("bsr_bf16_lds<c32,D4>", "bsr_bf16_lds<c32,D4>"),
    ("bsrc_mfma_bf16<c32>", "bsrc_mfma_bf16<c32>"),
    ("bsrc_slots_mfma_bf16<c32,nt,share>", "bsrc_slots_mfma_bf16<c32,nt,share>"),
    ("csr_f64<G32,V2,ref,wide> xcd 2x4", "csr_f64<G32,V2,ref,wide>"),
    ("csr_lds_tile<ref64,lds-dma> xcd 4x2, 21 tiles", "csr_lds_tile<ref64,lds-dma>"),
    ("csr_panel<fast,P128,R64,lds-dma> xcd 8x1, 3 panels", "csr_panel<fast,P128,R64,lds-dma>"),
    ("sddmm_csr<f64,ref,G64,V2,C0>", "sddmm_csr<f64,ref,G64,V2,C0>"),
    ("sddmm_bsr<b32,narrow,bf16,loop4>", "sddmm_bsr<b32,narrow,bf16,loop4>"),
    ("softmax_csr<f32,ref64,G4,R4>", "softmax_csr<f32,ref64,G4,R4>"),
    ("softmax_csr_bwd<f64,fast,G64,R4>", "softmax_csr_bwd<f64,fast,G64,R4>"),
    ("softmax_bsr<b16,bf16,walk,C32,mask>", "softmax_bsr<b16,bf16,walk,C32,mask>"),
    ("softmax_bsr_bwd<b32,f32,held,C16,p_bf16>", "softmax_bsr_bwd<b32,f32,held,C16,p_bf16>"),
]


@pytest.mark.parametrize("tag,key", EXAMPLES, ids=[t.split("<")[0] + str(i) for i, (t, _) in enumerate(EXAMPLES)])
def test_normalise_keeps_the_instance_and_drops_the_sizes(tag, key):
    assert census.normalise(tag) == key
    assert census.normalise(key.replace("+row_gather", " split 4 spans xcd 8x1 + row_gather")) == key      # idempotent
    assert census.parses(key)


def test_normalise_examples_cover_every_call_site():
    """One example per note_kernel format string of csrc/ (the <zero> memsets aside)."""
    src = os.path.join(capi.PKG_DIR, "csrc")
    heads = set()
    for name in os.listdir(src):
        with open(os.path.join(src, name), encoding="utf-8") as f:
            text = f.read()
        for fmt in re.findall(r'note_kernel\("([^"]*)"', text):
            if "<zero>" in fmt:
                continue
            if fmt.startswith("%s<"):                       # csr_wide / csr_k1 / csr_k2 share one call site
                heads |= {"csr_wide", "csr_k1", "csr_k2"}
            elif fmt.startswith("bsr_mfma_bf16%s"):
                heads |= {"bsr_mfma_bf16", "bsr_mfma_bf16_b32"}
            else:
                heads.add(re.match(r"[a-z0-9_]+", fmt).group(0))
    covered = {re.match(r"[a-z0-9_]+", t).group(0) for t, _ in EXAMPLES}
    assert heads == covered, (sorted(heads - covered), sorted(covered - heads))
    families = set(census.FAMILIES) | {"row_stream"}        # row_stream: the tuning build only, an exclusion
    assert heads == families, (sorted(heads - families), sorted(families - heads))


def test_xcd_of():
    assert census.xcd_of("row_gather<G16,V4,ref64,csr,B128,U8,roll,S16> xcd 1x8") == (1, 8)
    assert census.xcd_of("csr_k1<G8,V4,ref64>") is None


def test_tables_are_well_formed():
    assert sum(len(rows) for rows in census.FAMILIES.values()) > 400
    for family, rows in census.FAMILIES.items():
        keys = [r.key for r in rows]
        assert len(set(keys)) == len(keys), f"{family}: repeated keys {sorted(k for k in set(keys) if keys.count(k) > 1)}"
        for key in keys:
            assert census.parses(key), f"{family}: {key!r} is not what normalise returns"
            assert key.startswith(family + "<") or key == family, f"{family}: {key!r} belongs to another family"
            assert census.excluded(key) is None, f"{family}: {key!r} is in the table and matches the exclusion {census.excluded(key).pattern!r}"
    for e in census.EXCLUSIONS:
        assert e.why in census.REASONS and e.detail, e
    assert not census.FAMILIES["csr_wide"] and census.excluded("csr_wide<G8,V4,ref64>").why == "2gib"
    assert census.excluded("row_gather<G16,V4,ref64,uniform,B128,U8,roll,S14>").why == "2gib"
    assert census.excluded("row_stream<G16,ref64,uniform,W14>").why == "knob"


def test_the_fourteen_sddmm_instances_no_width_reached_before_are_in_the_table():
    rows = {r.key: r.spec for r in census.FAMILIES["sddmm_csr"]}
    assert len(rows) == 56
    for dt, accs, cases in (("f32", ("ref64", "fast"), (("G32,V4,C1", 128), ("G16,V1,C1", 13), ("G32,V1,C1", 27))),
                            ("f64", ("ref", "fast"), (("G16,V2,C1", 20), ("G64,V2,C1", 100), ("G16,V1,C1", 13), ("G32,V1,C1", 27)))):
        for acc in accs:
            for inst, n in cases:
                spec = rows[f"sddmm_csr<{dt},{acc},{inst}>"]
                assert spec["n"] == n and spec["acc"] == census.MODES[acc]


def _check_csr(csr, what):
    rp = np.asarray(csr.row_ptrs, dtype=np.int64)
    assert rp.shape == (csr.num_rows + 1,) and rp[0] == 0 and np.all(np.diff(rp) >= 0) and rp[-1] == csr.nnz == csr.data.shape[0], what
    assert csr.nnz == 0 or int(np.max(csr.col_idxs)) < csr.num_cols, what
    for r in range(csr.num_rows):
        assert np.all(np.diff(csr.col_idxs[rp[r]:rp[r + 1]].astype(np.int64)) > 0), f"{what}: row {r} does not ascend"


def _check_bsr(bsr, what):
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    assert bsr.num_rows % bsr.block_row_size == 0 and bsr.num_cols % bsr.block_col_size == 0, what
    assert ptrs.shape == (bsr.num_block_rows + 1,) and ptrs[0] == 0 and np.all(np.diff(ptrs) >= 0) and ptrs[-1] == bsr.num_blocks, what
    assert bsr.num_blocks == 0 or int(np.max(bsr.block_col_idxs)) < bsr.num_cols // bsr.block_col_size, what
    assert bsr.data.shape == (bsr.num_blocks, bsr.block_row_size, bsr.block_col_size), what


def test_every_builder_returns_operands_whose_indices_are_in_range():
    import _sddmm_bsr_ref as sbr
    import _softmax_bsr_ref as smb
    seen = 0
    for family, row in census.all_rows() + [("row_gather", census.Row(f"tiling {pq}", spec)) for pq, spec in census.ROW_GATHER_TILINGS.items()]:
        spec, what = row.spec, f"{family} {row.key}"
        if "pattern" in spec:
            _check_bsr((smb if family.startswith("softmax") else sbr).pattern(spec["pattern"]), what)
        elif "bs" in spec:
            host = census.bsr_operands(spec)
            _check_bsr(host["bsr"], what)
            assert host["b"].shape == (host["bsr"].num_cols, spec["n"]), what
        elif "g" in spec:
            ptr = census.softmax_csr_pattern(spec["g"]).astype(np.int64)
            assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and (np.diff(ptr) > 4 * spec["g"]).any() and (np.diff(ptr) == 0).any(), what
        else:
            host = census.spmm_operands(dict(spec, fmt=spec.get("fmt", "csr")))
            _check_csr(host["csr"], what)
            assert host["b"].shape == (host["csr"].num_cols, spec["n"]) and np.all(np.isfinite(host["b"])), what
            mean = host["csr"].nnz // host["csr"].num_rows
            assert (mean >= 24) == (spec["rows"] in ("long", "all-long")), f"{what}: mean row of {mean}"
            if isinstance(spec["rows"], int):
                assert np.all(np.diff(host["csr"].row_ptrs.astype(np.int64)) == spec["rows"]), what
            elif spec["rows"] in ("short", "long", "tail", "all-long") and family != "sddmm_csr":
                assert host["csr"].nnz % host["csr"].num_rows != 0, f"{what}: nnz divides by M (the general entry point would bet on uniform rows)"
        seen += 1
    assert seen == sum(len(r) for r in census.FAMILIES.values()) + 4


def _symbol_tool():
    for tool in ("nm", "llvm-nm"):
        path = shutil.which(tool)
        if path:
            return path
    for root in (os.environ.get("ROCM_PATH") or "/opt/rocm",):
        for sub in ("llvm/bin/llvm-nm", "lib/llvm/bin/llvm-nm", "bin/llvm-nm"):
            if os.path.exists(os.path.join(root, sub)):
                return os.path.join(root, sub)
    return None


def _symbols():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    assert os.path.exists(capi.LIB_PATH), f"{capi.LIB_PATH} is not built"
    return subprocess.run([tool, "-C", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_every_row_gather_instance_of_the_library_is_in_the_table_or_excluded():
    """The largest family, instance by instance: the template arguments of every row_gather_kernel / row_line_kernel
    instantiation spell a key (the store form aside); that key is a row of the table or falls under an exclusion, and every
    row of the table has its instantiation."""
    acc = {"AccRefWide": "ref64", "AccRefF32": "ref32", "AccFast": "fast"}
    rows = {"CsrRows": "csr", "UniformRows": "uniform", "SpanRows": "spans", "EllRows": "ell"}
    table = {r.key for r in census.FAMILIES["row_gather"]}
    met, loose = set(), set()
    for name, args in set(re.findall(r"__device_stub__(row_gather_kernel|row_line_kernel)<([^>]*)>", _symbols())):
        a = [s.strip().replace("mispmm::", "") for s in args.split(",")]
        if name == "row_gather_kernel":
            g, v, ac, _, rw, blk, u, roll, slots, batched, mapped = a
            if rw == "SpanRows":                   # the row-gather half of csr_hybrid is no kernel of its own
                continue
            key = f"row_gather<G{g},V{v},{acc[ac]},{rows[rw]},B{blk},U{u},{'roll' if roll == 'true' else 'batch'},S{slots}>"
        else:
            g, ac, padded, slots, batched, mapped = a
            key = f"row_gather<G{g},V4,{acc[ac]},{'ell' if padded == 'true' else 'uniform'},B128,U8,line,S{slots}>"
        key += (" batched" if batched == "true" else "") + (" plan-order" if mapped == "true" else "")
        if key in table:
            met.add(key)
        elif census.excluded(key) is None:
            loose.add(key)
    assert not loose, f"instances that are neither in the table nor excluded: {sorted(loose)}"
    assert met == table, f"rows of the table without an instantiation: {sorted(table - met)}"


def test_the_library_holds_the_recorded_number_of_instances_per_kernel_template():
    """__device_stub__ symbols of libmispmm.so by template name against census.INSTANCES.  A new or a lost instantiation fails
    here until someone has decided whether it is reachable and brought the tables, the exclusions and the count up to date."""
    out = _symbols()
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found, "no __device_stub__ symbol: was the library stripped?"
    differ = {k: (found.get(k, 0), census.INSTANCES.get(k, 0)) for k in set(found) | set(census.INSTANCES)
              if found.get(k, 0) != census.INSTANCES.get(k, 0)}
    assert not differ, f"kernel template: (instances in the library, recorded in tests/_census.py) {differ}"
