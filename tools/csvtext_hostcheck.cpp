// Host build of the CSV text core (sequoia-pub_amd/csrc/fmt_core.h) for tests/test_csvtext_host.py, which compiles this
// stand-alone program with the host compiler and the address and undefined-behaviour sanitizers and compares what it writes
// with numpy and pandas.      csvtext_hostcheck MODE IN OUT [CAPACITY]
//   f32   IN: uint32 bit patterns          OUT: the text of every float32, each followed by '\n' (NaN: an empty line)
//   i64   IN: int64 values                 OUT: the text of every value, each followed by '\n'
//   rows  IN: int64 n, n_int, n_f32; int64 index[n]; int64 ints[n][n_int]; float32 f32[n][n_f32]
//         OUT: the rows as sq_csv_format_rows lays them out -- pass 1 the length of every cell, an exclusive scan, pass 2 the
//         bytes, every byte below CAPACITY (default: the total) stored and none at or behind it, the part of a cell that
//         straddles it included -- in a buffer of exactly CAPACITY bytes.
// Every text is written into a heap block of exactly its length (one byte for an empty text), so a byte too many is the
// sanitizer's to report.
#include "../sequoia-pub_amd/csrc/fmt_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool read_file(const char* path, std::vector<char>& data) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    return true;
}

template <typename T, typename F>
static void values(const std::vector<char>& in, FILE* out, F text) {
    const size_t n = in.size() / sizeof(T);
    for (size_t i = 0; i < n; ++i) {
        T v;
        memcpy(&v, in.data() + i * sizeof(T), sizeof(T));
        const int len = text(v, (char*)nullptr, false);
        char* cell = (char*)malloc(len > 0 ? (size_t)len : 1);   // the text, not a byte more
        const int again = text(v, cell, true);
        if (again != len) { fprintf(stderr, "ERROR: value %zu: lengths %d and %d\n", i, len, again); exit(1); }
        fwrite(cell, 1, (size_t)len, out);
        fputc('\n', out);
        free(cell);
    }
}

static int rows(const std::vector<char>& in, FILE* out, long long capacity) {
    int64_t head[3];
    if (in.size() < sizeof head) return 2;
    memcpy(head, in.data(), sizeof head);
    const long long n = head[0];
    const int n_int = (int)head[1], n_f32 = (int)head[2];
    const size_t want = sizeof head + (size_t)n * 8 * (size_t)(1 + n_int) + (size_t)n * 4 * (size_t)n_f32;
    if (n < 0 || n_int < 0 || n_f32 < 0 || in.size() != want) return 2;
    std::vector<int64_t> index((size_t)n), ints((size_t)n * (size_t)n_int);
    std::vector<float> f32((size_t)n * (size_t)n_f32);
    const char* p = in.data() + sizeof head;
    if (n) memcpy(index.data(), p, index.size() * 8);
    p += index.size() * 8;
    if (!ints.empty()) memcpy(ints.data(), p, ints.size() * 8);
    p += ints.size() * 8;
    if (!f32.empty()) memcpy(f32.data(), p, f32.size() * 4);
    const SqfTable t = {index.data(), ints.data(), f32.data(), n_int, n_f32, (long long)n_f32};
    const int C = 1 + n_int + n_f32;
    const long long cells = n * C;
    std::vector<unsigned char> len((size_t)cells);
    std::vector<long long> off((size_t)cells + 1);
    for (long long c = 0; c < cells; ++c) len[(size_t)c] = (unsigned char)sqf_cell<false>(t, c / C, (int)(c % C), nullptr);
    off[0] = 0;
    for (long long c = 0; c < cells; ++c) off[(size_t)c + 1] = off[(size_t)c] + len[(size_t)c];
    const long long total = off[(size_t)cells];
    if (capacity < 0) capacity = total;
    char* text = (char*)malloc(capacity > 0 ? (size_t)capacity : 1);
    memset(text, '#', capacity > 0 ? (size_t)capacity : 1);
    for (long long c = 0; c < cells; ++c) {
        const long long at = off[(size_t)c];
        if (at >= capacity) break;
        int w;
        if (off[(size_t)c + 1] <= capacity) {
            w = sqf_cell<true>(t, c / C, (int)(c % C), text + at);
        } else {                                                 // the cell straddles the capacity: its image, then the bytes below it
            char* image = (char*)malloc(len[(size_t)c]);
            w = sqf_cell<true>(t, c / C, (int)(c % C), image);
            memcpy(text + at, image, (size_t)(capacity - at));
            free(image);
        }
        if (w != len[(size_t)c]) { fprintf(stderr, "ERROR: cell %lld: lengths %d and %d\n", c, (int)len[(size_t)c], w); return 1; }
    }
    fwrite(text, 1, (size_t)(total < capacity ? total : capacity), out);
    free(text);
    printf("%lld rows, %lld bytes, %s\n", n, total, total > capacity ? "overflow" : "ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "ERROR: usage: csvtext_hostcheck f32|i64|rows IN OUT [CAPACITY]\n"); return 2; }
    std::vector<char> in;
    if (!read_file(argv[2], in)) { fprintf(stderr, "ERROR: cannot read %s\n", argv[2]); return 2; }
    FILE* out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "ERROR: cannot write %s\n", argv[3]); return 2; }
    int rc = 0;
    const std::string mode = argv[1];
    if (mode == "f32") {
        values<uint32_t>(in, out, [](uint32_t v, char* o, bool w) { return w ? sqf_f32<true>(v, o) : sqf_f32<false>(v, o); });
    } else if (mode == "i64") {
        values<int64_t>(in, out, [](int64_t v, char* o, bool w) { return w ? sqf_i64<true>(v, o) : sqf_i64<false>(v, o); });
    } else if (mode == "rows") {
        rc = rows(in, out, argc > 4 ? atoll(argv[4]) : -1);
        if (rc == 2) fprintf(stderr, "ERROR: %s is no rows file\n", argv[2]);
    } else {
        fprintf(stderr, "ERROR: mode '%s'\n", argv[1]);
        rc = 2;
    }
    fclose(out);
    return rc;
}
