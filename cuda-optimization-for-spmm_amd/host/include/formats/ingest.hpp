// Reading the text formats without trusting them.  Every reader takes its tokens through TextFile, so that an index is
// range-checked as a signed 64-bit number before it becomes a uint32 ("-1" never wraps silently), a header that promises
// more than the file can hold is refused before anything is allocated, and every refusal is a std::runtime_error
// `<path>: malformed <kind> file: <what>` -- which main.cpp turns into `Error: ...` and exit status 1.
#pragma once

#include <cstdint>
#include <string>

namespace cuspmm {

class TextFile {
  public:
    // throws "cannot open <path>" (after the reference's "File ... doesn't exist!" line on stderr)
    TextFile(const std::string &path, const char *kind);
    [[noreturn]] void bad(const std::string &what) const;
    // a header field: an integer in 0 .. 2^32 - 1
    uint32_t count(const char *name);
    // element i of an index array: an integer in lowest .. 2^32 - 1, stored modulo 2^32 (lowest = -2^31 for the ELL index
    // files, whose "-1" is padding; 0 everywhere else)
    uint32_t index(const char *name, size_t i, long long lowest = 0);
    // element i of a value array; "nan" and "inf" are numbers
    template <typename DT> DT value(const char *name, size_t i);
    // a token needs at least two bytes (itself and a separator): refuse a header that promises more tokens than that
    void promise(uint64_t tokens) const;
    // the rest of the current line / the next whole line (false at the end of the file); for the line-oriented dense format
    bool line(std::string &out);
    // all of `line` as exactly `count` numbers into dst, else bad("row <row> ...")
    template <typename DT> void numbersOfLine(const std::string &line, size_t row, size_t count, DT *dst) const;
    size_t bytes() const { return text.size(); }

  private:
    bool token(const char *&begin, const char *&end);
    std::string path, kind, text;
    size_t at = 0;
};

// throws std::runtime_error("<origin>: <detail of the library's checker>") when a mispmm_*_check_host status is a refusal
void throwIfInvalid(int status, const std::string &origin);

}  // namespace cuspmm
