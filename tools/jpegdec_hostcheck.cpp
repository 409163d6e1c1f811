// Host check of the JPEG decode core: compiles sequoia-pub_amd/csrc/jpeg_core.h -- the text the device kernels are built
// from -- for the CPU and runs it over job files, so that the core's arithmetic can be compared with Pillow's bytes and its
// bounds checks can run under the host sanitizers (tests/test_wsi_host.py builds this with -fsanitize=address,undefined).
// It drives the core exactly as csrc/jpegdec.hip does: table derivation, the per-tile row check, the scan into zeroed
// coefficients, the IDCT into planes, and sqj_pixel for every pixel of every tile.
//
//   jpegdec_hostcheck <directory>
// For every <name>.job in the directory it writes <name>.out.  A job is little-endian:
//   int32 [12]   magic 0x4A51534A, tile_w, tile_h, hs, vs, transform, n_tiles, n_table_sets, scans_bytes, 0, 0, 0
//   int32 [n_tiles][SQ_JPEG_TILE_WORDS]   the tile table      uint8 [n_table_sets][SQ_JPEG_TABLE_SET_BYTES]   the table sets
//   uint8 [scans_bytes]                   the scans (scans_bytes a multiple of 16)
// and an output is int32 [n_tiles] statuses followed by uint8 [n_tiles][tile_h][tile_w][3] RGB.
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../sequoia-pub_amd/csrc/jpeg_core.h"

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
    if (!read_file(path, &raw) || raw.size() < 48) { fprintf(stderr, "%s: unreadable\n", path.c_str()); return 1; }
    int32_t head[12];
    memcpy(head, raw.data(), sizeof(head));
    const int tile_w = head[1], tile_h = head[2], hs = head[3], vs = head[4], transform = head[5], n_tiles = head[6], n_sets = head[7];
    const long long scans_bytes = head[8];
    SqjGeom g;
    if (head[0] != 0x4A51534A || !sqj_geom(tile_w, tile_h, hs, vs, &g) || n_tiles < 1 || n_tiles > 4096 || n_sets < 1 || n_sets > 4096 ||
        scans_bytes < 16 || scans_bytes % 16) { fprintf(stderr, "%s: bad header\n", path.c_str()); return 1; }
    const size_t table_at = 48, sets_at = table_at + (size_t)n_tiles * SQ_JPEG_TILE_WORDS * 4;
    const size_t scans_at = sets_at + (size_t)n_sets * SQ_JPEG_TABLE_SET_BYTES;
    if (raw.size() != scans_at + (size_t)scans_bytes) { fprintf(stderr, "%s: size does not match its header\n", path.c_str()); return 1; }
    // exact-size copies, so that the address sanitizer sees every access past an end
    std::vector<int32_t> table((size_t)n_tiles * SQ_JPEG_TILE_WORDS);
    memcpy(table.data(), raw.data() + table_at, table.size() * 4);
    std::vector<uint8_t> sets(raw.begin() + sets_at, raw.begin() + scans_at);
    std::vector<SqjChunk> scans((size_t)scans_bytes / 16);
    memcpy(scans.data(), raw.data() + scans_at, (size_t)scans_bytes);

    std::vector<SqjHuff> huff((size_t)n_sets * 4);
    std::vector<uint16_t> quant((size_t)n_sets * 4 * 64);
    for (int t = 0; t < n_sets * 4; t++) {
        const uint8_t* set = sets.data() + (size_t)(t >> 2) * SQ_JPEG_TABLE_SET_BYTES;
        sqj_build_huff(set + SQJ_QUANT_BYTES + (t & 3) * SQJ_HUFF_BYTES, (t & 3) < 2, &huff[t]);
        const uint8_t* q = set + (t & 3) * 128;
        for (int k = 0; k < 64; k++) quant[(size_t)t * 64 + sqj_zigzag(k)] = (uint16_t)(q[2 * k] | (q[2 * k + 1] << 8));
    }
    const uint8_t zigzag[64] = SQJ_ZIGZAG_INIT;
    std::vector<int32_t> status(n_tiles);
    std::vector<uint8_t> rgb((size_t)n_tiles * tile_h * tile_w * 3);
    std::vector<int16_t> coefs((size_t)g.blocks * 64);
    std::vector<uint8_t> planes((size_t)g.plane_bytes);
    for (int tile = 0; tile < n_tiles; tile++) {
        const int32_t* row = &table[(size_t)tile * SQ_JPEG_TILE_WORDS];
        std::fill(coefs.begin(), coefs.end(), (int16_t)0);
        int rc = sqj_tile_check(row, n_sets, (unsigned long long)scans_bytes, huff.data());
        if (rc == SQ_JPEG_OK)
            rc = sqj_scan(scans.data(), (uint32_t)row[0], (uint32_t)row[0] + (uint32_t)row[1], &g, &huff[(size_t)row[2] * 4], zigzag, row[4], row[3], coefs.data());
        status[tile] = rc;
        const bool have_q = row[2] >= 0 && row[2] < n_sets;
        const uint16_t zeros[64] = {0};
        for (int c = 0; c < 3; c++) {
            const int pw = c == 0 ? g.tile_w : g.cw, ph = c == 0 ? g.tile_h : g.ch;
            uint8_t* plane = planes.data() + (c == 0 ? 0 : (size_t)g.tile_w * g.tile_h + (size_t)(c - 1) * g.cw * g.ch);
            const uint16_t* q = have_q ? &quant[((size_t)row[2] * 4 + ((row[4] >> (4 * c)) & 3)) * 64] : zeros;
            for (int by = 0; by < ph / 8; by++)
                for (int bx = 0; bx < pw / 8; bx++)
                    sqj_idct_block(&coefs[(size_t)sqj_block_index(&g, c, bx, by) * 64], q, plane + (size_t)by * 8 * pw + bx * 8, pw);
        }
        uint8_t* dst = rgb.data() + (size_t)tile * tile_h * tile_w * 3;
        for (int y = 0; y < tile_h; y++)
            for (int x = 0; x < tile_w; x++) {
                const uint32_t px = sqj_pixel(planes.data(), &g, x, y, transform);
                dst[0] = (uint8_t)px; dst[1] = (uint8_t)(px >> 8); dst[2] = (uint8_t)(px >> 16);
                dst += 3;
            }
    }
    const std::string out = path.substr(0, path.size() - 4) + ".out";
    FILE* f = fopen(out.c_str(), "wb");
    if (!f) { fprintf(stderr, "%s: cannot write\n", out.c_str()); return 1; }
    fwrite(status.data(), 4, status.size(), f);
    fwrite(rgb.data(), 1, rgb.size(), f);
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
