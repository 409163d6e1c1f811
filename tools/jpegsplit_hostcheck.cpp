// Host check of the split (lane-parallel) JPEG entropy decode: compiles the lane-level functions of
// sequoia-pub_amd/csrc/jpeg_core.h -- the text jpeg_entropy_split_kernel is built from -- for the CPU and drives them as the
// kernel does, with the 64 lanes of a wave as a loop and the wave's votes, shuffles and scans as plain loops, so that the
// split decode can be compared byte for byte with the serial one (tools/jpegdec_hostcheck.cpp) and its bounds checks can run
// under the host sanitizers (tests/test_wsi_split_host.py builds this with -fsanitize=address,undefined).
//
//   jpegsplit_hostcheck <directory> <sub_bytes>      sub_bytes 0: SQ_JPEG_SPLIT_SUB_DEFAULT
// Job and output files are those of jpegdec_hostcheck (<name>.job -> <name>.out).  One text line per job goes to stdout:
//   <name>: sync_rounds <the most synchronisation rounds any round of 64 subsequences needed> fallbacks <tiles that took sqj_scan>
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../sequoia-pub_amd/csrc/jpeg_core.h"

static const int LANES = 64;

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

// One tile as one wave decodes it (jpeg_entropy_split_kernel): the tile's status; coefs is the tile's, zeroed.
static int split_tile(const SqjChunk* words, const int32_t* row, const SqjGeom* g, const SqjHuff* huff, const uint8_t* zigzag, int sub,
                      int16_t* coefs, int* max_sync, int* fallbacks) {
    const uint32_t pos = (uint32_t)row[0], end = pos + (uint32_t)row[1];
    const int sel = row[4], restart = row[3];
    const long long n_sub = ((long long)row[1] + sub - 1) / sub;
    bool done = false, bad = restart > 0;
    SqjState carry;
    carry.pos = pos; carry.bit = 0; carry.blk = 0; carry.k = 0; carry.valid = 1;
    uint32_t base = 0, pred[3] = {0, 0, 0};
    for (long long first = 0; first < n_sub && !done && !bad; first += LANES) {
        SqjState guess[LANES], start[LANES];
        SqjSubResult res[LANES];
        uint32_t sub_end[LANES];
        for (int l = 0; l < LANES; l++) {            // the speculative pass
            const unsigned long long at = (unsigned long long)pos + (unsigned long long)(first + l) * sub;
            sub_end[l] = (uint32_t)std::min<unsigned long long>(at + sub, end);
            guess[l] = l == 0 ? carry : sqj_sub_guess(words, pos, end, (uint32_t)std::min<unsigned long long>(at, end));
            start[l] = guess[l];
            sqj_sub_run(words, end, g, huff, zigzag, sel, &start[l], sub_end[l], false, 0, 0, 0, 0, coefs, &res[l]);
        }
        int rounds = 0;
        for (int r = 0; r < LANES - 1; r++) {        // synchronisation: lane r is exact after round r
            bool any = false;
            for (int l = LANES - 1; l >= 1; l--) {   // downwards: lane l reads what lane l - 1 had before this round
                if (first + l >= n_sub) continue;    // a lane behind the scan's end has nothing to agree on
                const SqjState next = res[l - 1].end.valid ? res[l - 1].end : guess[l];
                if (sqj_state_same(next, start[l])) continue;
                start[l] = next;
                sqj_sub_run(words, end, g, huff, zigzag, sel, &start[l], sub_end[l], false, 0, 0, 0, 0, coefs, &res[l]);
                any = true;
            }
            if (!any) break;
            rounds++;
        }
        *max_sync = std::max(*max_sync, rounds);
        uint32_t blocks0[LANES], p0[LANES], p1[LANES], p2[LANES];
        uint32_t blocks = base, s0 = pred[0], s1 = pred[1], s2 = pred[2];
        int last = LANES - 1;
        for (int l = 0; l < LANES; l++) {            // the exclusive scans and the vote
            blocks0[l] = blocks; p0[l] = s0; p1[l] = s1; p2[l] = s2;
            blocks += (uint32_t)res[l].blocks; s0 += res[l].dc0; s1 += res[l].dc1; s2 += res[l].dc2;
            if (blocks >= (uint32_t)g->blocks) { done = true; last = l; bad = blocks > (uint32_t)g->blocks; break; }
            if (!res[l].end.valid) { bad = true; break; }
        }
        if (bad) break;
        for (int l = 0; l <= last; l++) {            // the write pass
            SqjSubResult w;
            sqj_sub_run(words, end, g, huff, zigzag, sel, &start[l], sub_end[l], true, (int)blocks0[l], p0[l], p1[l], p2[l], coefs, &w);
            if (w.rc != SQ_JPEG_OK) bad = true;
        }
        if (!done && sqj_state_same(res[LANES - 1].end, carry)) bad = true;      // a marker in the scan: no lane can pass it
        carry = res[LANES - 1].end;
        base = blocks; pred[0] = s0; pred[1] = s1; pred[2] = s2;
    }
    if (done && !bad) return SQ_JPEG_OK;
    *fallbacks += 1;                                 // anything irregular: the serial scan's status and coefficients
    std::fill(coefs, coefs + (size_t)g->blocks * 64, (int16_t)0);
    return sqj_scan(words, pos, end, g, huff, zigzag, sel, restart, coefs);
}

static int run_job(const std::string& path, const std::string& name, int sub) {
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
    int max_sync = 0, fallbacks = 0;
    for (int tile = 0; tile < n_tiles; tile++) {
        const int32_t* row = &table[(size_t)tile * SQ_JPEG_TILE_WORDS];
        std::fill(coefs.begin(), coefs.end(), (int16_t)0);
        int rc = sqj_tile_check(row, n_sets, (unsigned long long)scans_bytes, huff.data());
        if (rc == SQ_JPEG_OK)
            rc = split_tile(scans.data(), row, &g, &huff[(size_t)row[2] * 4], zigzag, sub, coefs.data(), &max_sync, &fallbacks);
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
    printf("%s: sync_rounds %d fallbacks %d\n", name.substr(0, name.size() - 4).c_str(), max_sync, fallbacks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <directory of .job files> <sub_bytes, 0 for the default>\n", argv[0]); return 2; }
    int sub = atoi(argv[2]);
    if (sub == 0) sub = SQ_JPEG_SPLIT_SUB_DEFAULT;
    if (sub < SQ_JPEG_SPLIT_SUB_MIN || sub > SQ_JPEG_SPLIT_SUB_MAX || sub % 4) {
        fprintf(stderr, "sub_bytes = %s: a multiple of 4 in %d..%d, or 0\n", argv[2], SQ_JPEG_SPLIT_SUB_MIN, SQ_JPEG_SPLIT_SUB_MAX);
        return 2;
    }
    DIR* d = opendir(argv[1]);
    if (!d) { fprintf(stderr, "%s: not a directory\n", argv[1]); return 2; }
    int failed = 0, n = 0;
    while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".job") == 0) {
            failed += run_job(std::string(argv[1]) + "/" + name, name, sub);
            n++;
        }
    }
    closedir(d);
    printf("%d job(s), %d failed\n", n, failed);
    return failed ? 1 : 0;
}
