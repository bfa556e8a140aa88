#include "formats/ingest.hpp"

#include <cerrno>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "mispmm.h"

namespace cuspmm {

static bool isSpace(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

TextFile::TextFile(const std::string &path, const char *kind) : path(path), kind(kind) {
    std::ifstream in(path, std::ios::binary);
    if (!in.is_open()) {
        std::cerr << "File " << path << " doesn't exist!" << std::endl;
        throw std::runtime_error("cannot open " + path);
    }
    std::ostringstream all;
    all << in.rdbuf();
    text = all.str();
}

void TextFile::bad(const std::string &what) const { throw std::runtime_error(path + ": malformed " + kind + " file: " + what); }

bool TextFile::token(const char *&begin, const char *&end) {
    while (at < text.size() && isSpace(text[at])) ++at;
    if (at == text.size()) return false;
    const size_t start = at;
    while (at < text.size() && !isSpace(text[at])) ++at;
    begin = text.data() + start;
    end = text.data() + at;
    return true;
}

static std::string element(const char *name, size_t i) { return std::string(name) + "[" + std::to_string(i) + "]"; }

// [begin, end) as a whole integer; false if it is none or does not fit 64 bits
static bool wholeInteger(const char *begin, const char *end, long long &v) {
    char *stop = nullptr;
    errno = 0;
    v = std::strtoll(begin, &stop, 10);  // the text is NUL-terminated and a token holds no space: strtoll stops at `end` at the latest
    return stop == end && errno != ERANGE;
}

uint32_t TextFile::count(const char *name) {
    const char *b, *e;
    if (!token(b, e)) bad(std::string("truncated: the header ends before ") + name);
    long long v;
    if (!wholeInteger(b, e, v)) bad(std::string("header: ") + name + ": not a number: '" + std::string(b, e) + "'");
    if (v < 0 || v > 0xFFFFFFFFll) bad(std::string("header: ") + name + " = " + std::to_string(v) + " is not a count (0 .. 4294967295)");
    return (uint32_t)v;
}

uint32_t TextFile::index(const char *name, size_t i, long long lowest) {
    const char *b, *e;
    if (!token(b, e)) bad("truncated: " + std::string(name) + " ends after " + std::to_string(i) + " tokens");
    long long v;
    if (!wholeInteger(b, e, v)) bad(element(name, i) + ": not a number: '" + std::string(b, e) + "'");
    if (v < lowest || v > 0xFFFFFFFFll) bad(element(name, i) + " = " + std::to_string(v) + " is not an index");
    return (uint32_t)(unsigned long long)v;
}

template <typename DT> static bool wholeNumber(const char *begin, const char *end, DT &v) {
    char *stop = nullptr;
    if constexpr (sizeof(DT) == sizeof(float)) v = std::strtof(begin, &stop);
    else v = std::strtod(begin, &stop);
    return stop == end;
}

template <typename DT> DT TextFile::value(const char *name, size_t i) {
    const char *b, *e;
    if (!token(b, e)) bad("truncated: " + std::string(name) + " ends after " + std::to_string(i) + " tokens");
    DT v;
    if (!wholeNumber(b, e, v)) bad(element(name, i) + ": not a number: '" + std::string(b, e) + "'");
    return v;
}
template float TextFile::value<float>(const char *, size_t);
template double TextFile::value<double>(const char *, size_t);

void TextFile::promise(uint64_t tokens) const {
    if (tokens > ((uint64_t)text.size() + 1) / 2)
        bad("header promises " + std::to_string(tokens) + " tokens, the file has " + std::to_string(text.size()) + " bytes");
}

bool TextFile::line(std::string &out) {
    if (at >= text.size()) return false;
    size_t stop = text.find('\n', at);
    if (stop == std::string::npos) stop = text.size();
    out.assign(text, at, stop - at);
    at = stop < text.size() ? stop + 1 : stop;
    return true;
}

template <typename DT> void TextFile::numbersOfLine(const std::string &line, size_t row, size_t count, DT *dst) const {
    const std::string where = "row " + std::to_string(row);
    size_t p = 0, n = 0;
    for (;;) {
        while (p < line.size() && isSpace(line[p])) ++p;
        if (p == line.size()) break;
        const size_t start = p;
        while (p < line.size() && !isSpace(line[p])) ++p;
        const std::string tok = line.substr(start, p - start);
        DT v;
        if (!wholeNumber(tok.c_str(), tok.c_str() + tok.size(), v)) bad(where + ", token " + std::to_string(n) + ": not a number: '" + tok + "'");
        if (n < count) dst[n] = v;
        ++n;
    }
    if (n != count) bad(where + " holds " + std::to_string(n) + " tokens, " + std::to_string(count) + " are needed");
}
template void TextFile::numbersOfLine<float>(const std::string &, size_t, size_t, float *) const;
template void TextFile::numbersOfLine<double>(const std::string &, size_t, size_t, double *) const;

void throwIfInvalid(int status, const std::string &origin) {
    if (status == MISPMM_OK) return;
    const char *detail = mispmm_last_error();
    throw std::runtime_error(origin + ": " + ((detail && detail[0]) ? detail : mispmm_status_string(status)));
}

}  // namespace cuspmm
