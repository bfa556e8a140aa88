// The way in, under AddressSanitizer and UBSan, without a GPU (make ingest_san):
//   ingest_san <directory of malformed cases> <directory of valid cases>
// Each sub-directory is one case, laid out like a data directory of cuspmm: a sparse file (*.csr, *.coo, *.bsr, the
// column-major ELL pair *_rowind.ell + *_values_colmajor.ell, or the row-major pair *_colind.ell + *_values.ell) and a
// dense.in.  For every case the readers are constructed, as float and as double.  A refusal is printed.  An accepted matrix
// goes through toDense(), the sequential CPU engine of its format and every `_host` builder its copy2Device() would call.
// Exit status 0 only if every malformed case was refused by a reader, every valid case was accepted -- and no sanitizer
// spoke (a report ends the process with a status of its own).  Nothing here touches a device.
#include <algorithm>
#include <filesystem>
#include <memory>
#include <vector>

#include "engine.hpp"
#include "format.hpp"

using namespace cuspmm;
namespace fs = std::filesystem;

#define OK_OR_THROW(call) throwIfInvalid((call), #call)

struct CaseFiles {
    std::string dir, csr, coo, bsr, rowind, valuesCm, colind, valuesRm, dense;
};

static CaseFiles findFiles(const fs::path &dir) {
    CaseFiles f;
    f.dir = dir.string();
    for (const auto &entry : fs::directory_iterator(dir)) {
        const std::string name = entry.path().filename().string(), path = entry.path().string();
        if (endsWith(name, ".coo")) f.coo = path;
        else if (endsWith(name, ".csr")) f.csr = path;
        else if (endsWith(name, ".bsr")) f.bsr = path;
        else if (endsWith(name, "_colind.ell")) f.colind = path;
        else if (endsWith(name, "_values.ell")) f.valuesRm = path;
        else if (endsWith(name, "_rowind.ell")) f.rowind = path;
        else if (endsWith(name, "_values_colmajor.ell")) f.valuesCm = path;
        else if (endsWith(name, "dense.in")) f.dense = path;
    }
    return f;
}

// the span list of a row-pointer array, both ways copy2Device() asks for it, and where its long rows end
static void spansOf(uint32_t numRows, const uint32_t *rowPtrs) {
    for (uint32_t shareLen : {0u, 0xFFFFFFFFu}) {
        uint32_t count = 0, numLong = 0;
        OK_OR_THROW(mispmm_csr_spans_by_length_host(numRows, rowPtrs, shareLen, &count, nullptr));
        std::vector<uint32_t> spans((size_t)count * 4 + 1);
        OK_OR_THROW(mispmm_csr_spans_by_length_host(numRows, rowPtrs, shareLen, &count, spans.data()));
        OK_OR_THROW(mispmm_csr_spans_long_count_host(count, spans.data(), 32, &numLong));
    }
}

template <typename Engine, typename Mat, typename DT> static void cpuProduct(const CaseFiles &f, Mat &a, DenseMatrix<DT, uint32_t> &b) {
    if (a.numCols != b.numRows) throw std::runtime_error("A has " + std::to_string(a.numCols) + " columns, B " + std::to_string(b.numRows) + " rows");
    std::unique_ptr<DenseMatrix<DT, uint32_t>> dense(a.toDense());
    DenseMatrix<DT, uint32_t> c(a.numRows, b.numCols, false);
    Engine engine(f.dir);
    engine.runKernel(0, &a, &b, &c);
}

template <typename DT> static void runCsr(const CaseFiles &f) {
    SparseMatrixCSR<DT, uint32_t> a(f.csr);
    DenseMatrix<DT, uint32_t> b(f.dense);
    cpuProduct<EngineCSR<DT, uint32_t, double>>(f, a, b);
    a.validate("CSR, as copy2Device begins");
    spansOf(a.numRows, a.rowPtrs);
    if constexpr (std::is_same_v<DT, float>) {
        std::vector<uint32_t> order(a.numRows + 1), ptrs((size_t)a.numRows + 1), cols(a.numNonZero + 1), tptrs((size_t)a.numCols + 1), perm(a.numNonZero + 1);
        std::vector<float> vals(a.numNonZero + 1);
        uint64_t natural = 0, clustered = 0;
        OK_OR_THROW(mispmm_csr_cluster_rows_host(a.numRows, a.numCols, a.rowPtrs, a.colIdxs, 8, order.data(), &natural, &clustered));
        OK_OR_THROW(mispmm_csr_permute_rows_host(a.numRows, a.rowPtrs, a.colIdxs, a.data, order.data(), ptrs.data(), cols.data(), vals.data()));
        OK_OR_THROW(mispmm_csr_transpose_host(a.numRows, a.numCols, a.numNonZero, a.rowPtrs, a.colIdxs, tptrs.data(), cols.data(), perm.data()));
    }
}

template <typename DT> static void runCoo(const CaseFiles &f) {
    SparseMatrixCOO<DT, uint32_t> a(f.coo);
    DenseMatrix<DT, uint32_t> b(f.dense);
    cpuProduct<EngineCOO<DT, uint32_t, double>>(f, a, b);
    a.validate("COO, as copy2Device begins");
    // the row boundaries copy2Device() counts, then their span list
    std::vector<uint32_t> rp((size_t)a.numRows + 1, 0);
    for (size_t i = 0; i < a.numNonZero; ++i) ++rp[(size_t)a.rowIdxs[i] + 1];
    for (size_t r = 0; r < a.numRows; ++r) rp[r + 1] += rp[r];
    spansOf(a.numRows, rp.data());
    if constexpr (std::is_same_v<DT, float>) {
        std::vector<uint32_t> rows(a.numNonZero + 1), cols(a.numNonZero + 1);
        std::vector<float> vals(a.numNonZero + 1);
        int sorted = 0;
        OK_OR_THROW(mispmm_coo_sort_by_row_host(a.numRows, a.numNonZero, a.rowIdxs, a.colIdxs, a.data, rows.data(), cols.data(), vals.data(), &sorted));
    }
}

template <typename DT> static void runBsr(const CaseFiles &f) {
    SparseMatrixBSR<DT, uint32_t> a(f.bsr);
    DenseMatrix<DT, uint32_t> b(f.dense);
    cpuProduct<EngineBSR<DT, uint32_t, double>>(f, a, b);
    a.validate("BSR, as copy2Device begins");
    uint32_t nz = 0;
    std::vector<uint32_t> rp((size_t)a.numRows + 1);
    auto list = [&](auto builder) {
        OK_OR_THROW(builder(a.numBlockRows, a.blockRowSize, a.blockColSize, a.numBlocks, a.blockRowPtrs, a.blockColIdxs, a.data, &nz, nullptr, nullptr, nullptr));
        std::vector<uint32_t> ci(nz + 1);
        std::vector<DT> va(nz + 1);
        OK_OR_THROW(builder(a.numBlockRows, a.blockRowSize, a.blockColSize, a.numBlocks, a.blockRowPtrs, a.blockColIdxs, a.data, &nz, rp.data(), ci.data(), va.data()));
        for (uint32_t i = 0; i < nz; ++i)
            if (ci[i] >= a.numCols) throw std::runtime_error("bsr nonzeros built a column past K");
    };
    if constexpr (std::is_same_v<DT, float>) list(mispmm_bsr_nonzeros_host);
    else list(mispmm_bsr_nonzeros_f64_host);
    spansOf(a.numRows, rp.data());
}

template <typename DT> static void runEllColMajor(const CaseFiles &f) {
    SparseMatrixELL<DT, uint32_t> a(f.rowind, f.valuesCm);
    DenseMatrix<DT, uint32_t> b(f.dense);
    cpuProduct<EngineELL<DT, uint32_t, double>>(f, a, b);
    a.validate("ELL, as copy2Device begins");
    std::vector<uint32_t> rp((size_t)a.numRows + 1);
    uint32_t occupied = 0;
    if constexpr (std::is_same_v<DT, float>) {
        uint32_t width = 0;
        OK_OR_THROW(mispmm_ell_colmajor_to_rowmajor_host(a.numRows, a.numCols, a.maxColNnz, a.rowIdxs, a.data, &width, nullptr, nullptr));
        const size_t n = (size_t)a.numRows * width;
        std::vector<uint32_t> cols(n + 1);
        std::vector<float> vals(n + 1);
        OK_OR_THROW(mispmm_ell_colmajor_to_rowmajor_host(a.numRows, a.numCols, a.maxColNnz, a.rowIdxs, a.data, &width, cols.data(), vals.data()));
        OK_OR_THROW(mispmm_ell_check_host(MISPMM_ELL_ROW_MAJOR, a.numRows, a.numCols, width, cols.data(), n));
        OK_OR_THROW(mispmm_ell_compact_host(a.numRows, width, cols.data(), vals.data(), &occupied, nullptr, nullptr, nullptr));
        std::vector<uint32_t> ci(occupied + 1);
        std::vector<float> va(occupied + 1);
        OK_OR_THROW(mispmm_ell_compact_host(a.numRows, width, cols.data(), vals.data(), &occupied, rp.data(), ci.data(), va.data()));
    } else {
        OK_OR_THROW(mispmm_ell_colmajor_to_rows_f64_host(a.numRows, a.numCols, a.maxColNnz, a.rowIdxs, a.data, &occupied, nullptr, nullptr, nullptr));
        std::vector<uint32_t> ci(occupied + 1);
        std::vector<double> va(occupied + 1);
        OK_OR_THROW(mispmm_ell_colmajor_to_rows_f64_host(a.numRows, a.numCols, a.maxColNnz, a.rowIdxs, a.data, &occupied, rp.data(), ci.data(), va.data()));
    }
    spansOf(a.numRows, rp.data());
}

// The host layer has no class for the row-major pair (the command line loads the column-major one): the same token reader,
// the library's check for that layout, then the builder an upload of such arrays calls.
static void runEllRowMajor(const CaseFiles &f) {
    TextFile idx(f.colind, "ELL"), val(f.valuesRm, "ELL");
    const uint32_t numRows = idx.count("numRows"), numCols = idx.count("numCols");
    idx.count("numNonZero");
    const uint32_t width = idx.count("width");
    const uint64_t slots = (uint64_t)numRows * width;
    idx.promise(4 + slots);
    val.promise(slots);
    std::vector<uint32_t> cols(slots + 1), rp((size_t)numRows + 1);
    std::vector<float> vals(slots + 1);
    for (size_t i = 0; i < slots; ++i) cols[i] = idx.index("colIdxs", i, -0x80000000ll);
    for (size_t i = 0; i < slots; ++i) vals[i] = val.value<float>("data", i);
    throwIfInvalid(mispmm_ell_check_host(MISPMM_ELL_ROW_MAJOR, numRows, numCols, width, cols.data(), slots), f.colind + ": malformed ELL file");
    uint32_t occupied = 0;
    OK_OR_THROW(mispmm_ell_compact_host(numRows, width, cols.data(), vals.data(), &occupied, nullptr, nullptr, nullptr));
    std::vector<uint32_t> ci(occupied + 1);
    std::vector<float> va(occupied + 1);
    OK_OR_THROW(mispmm_ell_compact_host(numRows, width, cols.data(), vals.data(), &occupied, rp.data(), ci.data(), va.data()));
    spansOf(numRows, rp.data());
}

// true = accepted all the way through; false = refused (the message is printed)
static bool runCase(const CaseFiles &f) {
    try {
        if (!f.csr.empty()) runCsr<float>(f), runCsr<double>(f);
        if (!f.coo.empty()) runCoo<float>(f), runCoo<double>(f);
        if (!f.bsr.empty()) runBsr<float>(f), runBsr<double>(f);
        if (!f.rowind.empty()) runEllColMajor<float>(f), runEllColMajor<double>(f);
        if (!f.colind.empty()) runEllRowMajor(f);
        return true;
    } catch (const std::exception &e) {
        std::printf("  refused: %s\n", e.what());
        return false;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <directory of malformed cases> <directory of valid cases>\n", argv[0]);
        return 2;
    }
    int wrong = 0, count[2] = {0, 0};
    for (int valid = 0; valid < 2; ++valid) {
        std::vector<fs::path> cases;
        for (const auto &entry : fs::directory_iterator(argv[1 + valid]))
            if (entry.is_directory()) cases.push_back(entry.path());
        std::sort(cases.begin(), cases.end());
        for (const auto &dir : cases) {
            std::printf("%s %s\n", valid ? "valid    " : "malformed", dir.filename().c_str());
            const bool accepted = runCase(findFiles(dir));
            ++count[valid];
            if (accepted != (valid == 1)) {
                std::printf("  WRONG: %s\n", valid ? "a valid case was refused" : "a malformed case was accepted");
                ++wrong;
            }
        }
    }
    std::printf("ingest_san: %d malformed cases, %d valid cases, %d wrong verdicts\n", count[0], count[1], wrong);
    std::fflush(stdout);
    return wrong || count[0] == 0 || count[1] == 0 ? 1 : 0;
}
