#include "formats/sparse_ell.hpp"

#include <vector>

namespace cuspmm {

template <typename DT, typename MT>
SparseMatrixELL<DT, MT>::SparseMatrixELL(std::string rowindPath, std::string valuesPath) {
    TextFile idx(rowindPath, "ELL"), val(valuesPath, "ELL");
    this->numRows = idx.count("numRows");
    this->numCols = idx.count("numCols");
    this->numNonZero = idx.count("numNonZero");
    this->maxColNnz = idx.count("maxColNnz");
    const size_t slots = this->numSlots();
    idx.promise(4 + (uint64_t)slots);
    val.promise(slots);
    this->allocateSpace(false);
    try {
        // "-1" marks padding; stored as 0xFFFFFFFF like `istream >> uint32_t` does.  Any index with the sign bit set is padding
        // (the reference's `if (row >= 0)`), so the tokens may go down to -2^31; the structure check decides about the others.
        for (size_t i = 0; i < slots; ++i) this->rowIdxs[i] = idx.index("rowIdxs", i, -0x80000000ll);
        for (size_t i = 0; i < slots; ++i) this->data[i] = val.template value<DT>("data", i);
        this->validate(rowindPath + ": malformed ELL file");
    } catch (...) {
        this->release();  // a constructor that throws runs no destructor
        throw;
    }
}

template <typename DT, typename MT> void SparseMatrixELL<DT, MT>::validate(const std::string &origin) const {
    if (this->onDevice) throw std::runtime_error(origin + ": the structure check reads host arrays");
    throwIfInvalid(mispmm_ell_check_host(MISPMM_ELL_COLUMN_MAJOR, this->numRows, this->numCols, this->maxColNnz, this->rowIdxs, this->numSlots()),
                   origin);
}

template <typename DT, typename MT>
SparseMatrixELL<DT, MT>::SparseMatrixELL(MT numRows, MT numCols, MT numNonZero, MT maxColNnz, bool onDevice) {
    this->numRows = numRows;
    this->numCols = numCols;
    this->numNonZero = numNonZero;
    this->maxColNnz = maxColNnz;
    this->allocateSpace(onDevice);
}

template <typename DT, typename MT> SparseMatrixELL<DT, MT>::~SparseMatrixELL() { this->release(); }

template <typename DT, typename MT> void SparseMatrixELL<DT, MT>::release() {
    releaseBuffer(this->rowIdxs, this->onDevice);
    releaseBuffer(this->data, this->onDevice);
    releaseBuffer(this->rmColIdxs, true);
    releaseBuffer(this->rmData, true);
    releaseBuffer(this->cpRowPtrs, true);
    releaseBuffer(this->cpColIdxs, true);
    releaseBuffer(this->cpData, true);
    releaseBuffer(this->cpSpans, true);
    this->rowIdxs = this->rmColIdxs = this->cpRowPtrs = this->cpColIdxs = this->cpSpans = nullptr;
    this->data = this->rmData = this->cpData = nullptr;
}

template <typename DT, typename MT> bool SparseMatrixELL<DT, MT>::allocateSpace(bool onDevice) {
    assert(this->data == nullptr && this->rowIdxs == nullptr);
    this->rowIdxs = allocateBuffer<MT>(this->numSlots(), onDevice);
    this->data = allocateBuffer<DT>(this->numSlots(), onDevice);
    this->onDevice = onDevice;
    return true;
}

template <typename DT, typename MT> SparseMatrixELL<DT, MT> *SparseMatrixELL<DT, MT>::copy2Device() {
    this->validate("ELL copy2Device");  // before any device allocation: covers matrices filled in memory through the class API
    assert(!this->onDevice && this->data != nullptr);
    auto *d = new SparseMatrixELL<DT, MT>(this->numRows, this->numCols, this->numNonZero, this->maxColNnz, true);
    copyBuffer(d->rowIdxs, true, this->rowIdxs, false, this->numSlots() * sizeof(MT));
    copyBuffer(d->data, true, this->data, false, this->numSlots() * sizeof(DT));
    // Row-major view for the row-parallel kernel, built once here (layout conversion sits outside
    // the timed sections, like DenseMatrix::toOrdering in the reference's wrappers).
    if constexpr (std::is_same_v<DT, float>) {
        uint32_t width = 0;
        mispmmCheckError(mispmm_ell_colmajor_to_rowmajor_host(this->numRows, this->numCols, this->maxColNnz,
                                                              this->rowIdxs, this->data, &width, nullptr, nullptr));
        const size_t n = (size_t)this->numRows * width;
        std::vector<uint32_t> cols(n ? n : 1);
        std::vector<float> vals(n ? n : 1);
        mispmmCheckError(mispmm_ell_colmajor_to_rowmajor_host(this->numRows, this->numCols, this->maxColNnz,
                                                              this->rowIdxs, this->data, &width, cols.data(),
                                                              vals.data()));
        d->rowWidth = width;
        d->rmColIdxs = allocateBuffer<MT>(n, true);
        d->rmData = allocateBuffer<DT>(n, true);
        copyBuffer(d->rmColIdxs, true, cols.data(), false, n * sizeof(MT));
        copyBuffer(d->rmData, true, vals.data(), false, n * sizeof(DT));
        // mostly padding (an ELL is as wide as its longest row): also keep the list of occupied slots
        uint32_t occupied = 0;
        mispmmCheckError(mispmm_ell_compact_host(this->numRows, width, cols.data(), vals.data(), &occupied, nullptr, nullptr, nullptr));
        if (n != 0 && (size_t)occupied * 2 < n) {
            std::vector<uint32_t> rp((size_t)this->numRows + 1), ci(occupied ? occupied : 1);
            std::vector<float> va(occupied ? occupied : 1);
            mispmmCheckError(mispmm_ell_compact_host(this->numRows, width, cols.data(), vals.data(), &occupied, rp.data(), ci.data(),
                                                     va.data()));
            d->cpRowPtrs = allocateBuffer<MT>((size_t)this->numRows + 1, true);
            d->cpColIdxs = allocateBuffer<MT>(ci.size(), true);
            d->cpData = allocateBuffer<DT>(va.size(), true);
            copyBuffer(d->cpRowPtrs, true, rp.data(), false, rp.size() * sizeof(MT));
            copyBuffer(d->cpColIdxs, true, ci.data(), false, ci.size() * sizeof(MT));
            copyBuffer(d->cpData, true, va.data(), false, va.size() * sizeof(DT));
            d->cpCount = occupied;
            bool hybridOnly = false;
            if (wantsRowSpans(this->numRows, rp.data(), hybridOnly)) {
                uint32_t count = 0;
                uint32_t longCount = 0;
                d->cpSpans = uploadRowSpans(this->numRows, rp.data(), 0xFFFFFFFFu, count, &longCount);
                d->cpSpansLong = longCount;
                d->cpSpansHybridOnly = hybridOnly;
            }
        }
    } else {
        // fp64: the occupied slots straight from the column-major arrays as one row list, in spmmELLCpu's order
        // (mispmm_csr_f64 multiplies from it); no padded view, no span list
        uint32_t occupied = 0;
        mispmmCheckError(mispmm_ell_colmajor_to_rows_f64_host(this->numRows, this->numCols, this->maxColNnz, this->rowIdxs, this->data,
                                                              &occupied, nullptr, nullptr, nullptr));
        std::vector<uint32_t> rp((size_t)this->numRows + 1), ci(occupied ? occupied : 1);
        std::vector<double> va(occupied ? occupied : 1);
        mispmmCheckError(mispmm_ell_colmajor_to_rows_f64_host(this->numRows, this->numCols, this->maxColNnz, this->rowIdxs, this->data,
                                                              &occupied, rp.data(), ci.data(), va.data()));
        d->cpRowPtrs = allocateBuffer<MT>(rp.size(), true);
        d->cpColIdxs = allocateBuffer<MT>(ci.size(), true);
        d->cpData = allocateBuffer<DT>(va.size(), true);
        copyBuffer(d->cpRowPtrs, true, rp.data(), false, rp.size() * sizeof(MT));
        copyBuffer(d->cpColIdxs, true, ci.data(), false, ci.size() * sizeof(MT));
        copyBuffer(d->cpData, true, va.data(), false, va.size() * sizeof(DT));
        d->cpCount = occupied;
    }
    return d;
}

template <typename DT, typename MT> DenseMatrix<DT, MT> *SparseMatrixELL<DT, MT>::toDense() {
    assert(!this->onDevice);
    auto *dm = new DenseMatrix<DT, MT>(this->numRows, this->numCols, false);
    for (MT c = 0; c < this->numCols; ++c)
        for (MT s = 0; s < this->maxColNnz; ++s) {
            const size_t i = (size_t)c * this->maxColNnz + s;
            if ((int32_t)this->rowIdxs[i] >= 0) dm->data[RowMjIdx(this->rowIdxs[i], c, this->numCols)] = this->data[i];
        }
    return dm;
}

template class SparseMatrixELL<float, uint32_t>;
template class SparseMatrixELL<double, uint32_t>;

}  // namespace cuspmm
