// Host check of the TIFF LZW decode core: compiles sequoia-pub_amd/csrc/lzw_core.h -- the text the device kernels are built
// from -- for the CPU and runs it over job files, so that the core can be compared with libtiff's bytes and its bounds checks
// can run under the host sanitizers (tests/test_tiffz_host.py builds this plain and with -fsanitize=address,undefined).
// It drives the core as the lane mode of csrc/tifflzw.hip does: per tile the range check, the serial decoder into the tile's
// chunky bytes, then the predictor and the split into planes; an uncompressed tile is its bytes.
//
//   lzw_hostcheck <directory>
// For every <name>.job in the directory it writes <name>.out.  A job is little-endian:
//   int32 [8]   magic 0x575A4C53, tile_w, tile_h, n_tiles, scans_bytes, compression (5, 1), predictor (1, 2), 0
//   int32 [n_tiles][SQ_LZW_TILE_WORDS]   the tile table      uint8 [scans_bytes]   the tile bytes (a multiple of 16)
// and an output is int32 [n_tiles] statuses followed by uint8 [n_tiles][3][tile_h][tile_w] planes.
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../sequoia-pub_amd/csrc/lzw_core.h"

static bool read_file(const std::string& path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out->resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && fread(out->data(), 1, out->size(), f) == out->size();
    fclose(f);
    return ok;
}

static int run_job(const std::string& path) {
    std::vector<uint8_t> raw;
    if (!read_file(path, &raw) || raw.size() < 32) { fprintf(stderr, "%s: unreadable\n", path.c_str()); return 1; }
    int32_t head[8];
    memcpy(head, raw.data(), sizeof(head));
    const int tile_w = head[1], tile_h = head[2], n_tiles = head[3], compression = head[5], predictor = head[6];
    const long long scans_bytes = head[4];
    if (head[0] != 0x575A4C53 || tile_w < 16 || tile_w > SQ_JPEG_MAX_TILE || tile_h < 16 || tile_h > SQ_JPEG_MAX_TILE || (tile_w & 15) || (tile_h & 15) ||
        n_tiles < 1 || n_tiles > 4096 || scans_bytes < 16 || scans_bytes % 16 || (compression != 1 && compression != 5) ||
        (predictor != 1 && predictor != 2)) {
        fprintf(stderr, "%s: bad header\n", path.c_str());
        return 1;
    }
    const size_t table_at = 32, scans_at = table_at + (size_t)n_tiles * SQ_LZW_TILE_WORDS * 4;
    if (raw.size() != scans_at + (size_t)scans_bytes) { fprintf(stderr, "%s: size does not match its header\n", path.c_str()); return 1; }
    std::vector<int32_t> table((size_t)n_tiles * SQ_LZW_TILE_WORDS);
    memcpy(table.data(), raw.data() + table_at, table.size() * 4);

    const size_t plane = (size_t)tile_w * tile_h, total = 3 * plane;
    std::vector<int32_t> status(n_tiles);
    std::vector<uint8_t> planes((size_t)n_tiles * total, 0);
    for (int tile = 0; tile < n_tiles; tile++) {
        const int32_t* row = &table[(size_t)tile * SQ_LZW_TILE_WORDS];
        int rc = lzw_range_status(row, (unsigned long long)scans_bytes);
        if (rc == SQ_LZW_OK) {
            // exact-size copies, so that the address sanitizer sees every access past an end
            std::vector<uint8_t> scan(raw.begin() + scans_at + row[0], raw.begin() + scans_at + row[0] + row[1]);
            std::vector<uint8_t> chunky(total, 0);
            if (compression == 1) {
                if (scan.size() < total) rc = SQ_LZW_TRUNCATED;
                else memcpy(chunky.data(), scan.data(), total);
            } else {
                std::vector<LzwEntry> entries(LZW_TABLE_CODES);
                rc = lzw_decode_serial(scan.data(), (uint32_t)scan.size(), chunky.data(), (uint32_t)total, entries.data());
            }
            if (rc == SQ_LZW_OK) lzw_planes_serial(chunky.data(), tile_w, tile_h, predictor, planes.data() + (size_t)tile * total);
        }
        status[tile] = rc;
    }
    const std::string out = path.substr(0, path.size() - 4) + ".out";
    FILE* f = fopen(out.c_str(), "wb");
    if (!f) { fprintf(stderr, "%s: cannot write\n", out.c_str()); return 1; }
    fwrite(status.data(), 4, status.size(), f);
    fwrite(planes.data(), 1, planes.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <directory of .job files>\n", argv[0]); return 2; }
    DIR* d = opendir(argv[1]);
    if (!d) { fprintf(stderr, "%s: not a directory\n", argv[1]); return 2; }
    int failed = 0, n = 0;
    while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".job") == 0) {
            failed += run_job(std::string(argv[1]) + "/" + name);
            n++;
        }
    }
    closedir(d);
    printf("%d job(s), %d failed\n", n, failed);
    return failed ? 1 : 0;
}
