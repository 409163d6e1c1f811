// Host check of the JPEG 2000 decode core: compiles sequoia-pub_amd/csrc/j2k_core.h -- the text the device kernels are built
// from -- for the CPU and runs it over job files, so that the core can be compared with Pillow's bytes and its bounds checks
// can run under the host sanitizers (tests/test_j2k_host.py builds this with -fsanitize=address,undefined -ffp-contract=off).
// It drives the core exactly as csrc/j2kdec.hip does: per tile the packet walk into the tile's records, every code-block into
// zeroed samples, dequantisation into the component planes, the inverse wavelet, and j2k_pixel for every pixel.
//
//   j2k_hostcheck <directory> [--hits]
// For every <name>.job in the directory it writes <name>.out.  A job is little-endian:
//   int32 [12]   magic 0x4B324A4A, tile_w, tile_h, n_tiles, n_param_sets, streams_bytes, max_blocks, max_nodes, max_bands, 0, 0, 0
//   int32 [n_tiles][SQ_J2K_TILE_WORDS]   the tile table      uint8 [n_param_sets][SQ_J2K_PARAM_BYTES]   the parameter sets
//   uint8 [streams_bytes]                the packet bytes (streams_bytes a multiple of 16)
// and an output is int32 [n_tiles] statuses followed by uint8 [n_tiles][3][tile_h][tile_w] planes.  --hits prints how often
// each of the 19 MQ contexts was used over all jobs (tests/golden/make_j2k_golden.py asserts the noise case reaches all).
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

static unsigned long long g_hits[19];
#define J2K_HIT(cx) (g_hits[cx]++)
#include "../sequoia-pub_amd/csrc/j2k_core.h"

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
    const int tile_w = head[1], tile_h = head[2], n_tiles = head[3], n_sets = head[4];
    const long long streams_bytes = head[5];
    J2kCounts cap;
    cap.blocks = head[6]; cap.nodes = head[7]; cap.bands = head[8];
    if (head[0] != 0x4B324A4A || tile_w < 16 || tile_w > SQ_JPEG_MAX_TILE || tile_h < 16 || tile_h > SQ_JPEG_MAX_TILE || (tile_w & 15) || (tile_h & 15) ||
        n_tiles < 1 || n_tiles > 4096 || n_sets < 1 || n_sets > 4096 || streams_bytes < 16 || streams_bytes % 16 || cap.blocks < 1 ||
        cap.blocks > (1 << 20) || cap.nodes < 1 || cap.nodes > (1 << 22) || cap.bands < 1 || cap.bands > (1 << 20)) {
        fprintf(stderr, "%s: bad header\n", path.c_str());
        return 1;
    }
    const size_t table_at = 48, sets_at = table_at + (size_t)n_tiles * SQ_J2K_TILE_WORDS * 4;
    const size_t streams_at = sets_at + (size_t)n_sets * SQ_J2K_PARAM_BYTES;
    if (raw.size() != streams_at + (size_t)streams_bytes) { fprintf(stderr, "%s: size does not match its header\n", path.c_str()); return 1; }
    // exact-size copies, so that the address sanitizer sees every access past an end
    std::vector<int32_t> table((size_t)n_tiles * SQ_J2K_TILE_WORDS);
    memcpy(table.data(), raw.data() + table_at, table.size() * 4);
    std::vector<uint8_t> sets(raw.begin() + sets_at, raw.begin() + streams_at);
    std::vector<uint8_t> streams(raw.begin() + streams_at, raw.end());
    std::vector<uint8_t> gather((size_t)streams_bytes);

    const uint32_t mq_table[J2K_MQ_STATES] = J2K_MQ_TABLE_INIT;
    const size_t plane = (size_t)tile_w * tile_h;
    std::vector<int32_t> status(n_tiles);
    std::vector<uint8_t> planes((size_t)n_tiles * 3 * plane, 0);
    for (int tile = 0; tile < n_tiles; tile++) {
        J2kTile T;
        std::vector<J2kBand> bands(cap.bands);
        std::vector<J2kBlock> blocks(cap.blocks);
        std::vector<J2kNode> nodes(cap.nodes);
        const int rc = j2k_tile_packets(sets.data(), n_sets, &table[(size_t)tile * SQ_J2K_TILE_WORDS], streams.data(), (unsigned long long)streams_bytes,
                                        tile_w, tile_h, &cap, &T, bands.data(), blocks.data(), nodes.data(), gather.data());
        status[tile] = T.status = rc;
        if (rc != SQ_J2K_OK) continue;
        std::vector<int32_t> coef(3 * plane, 0), tmp(3 * plane, 0);
        for (int b = 0; b < T.n_blocks; b++) {
            const J2kBlock& K = blocks[b];
            std::vector<uint32_t> v((size_t)K.w * K.h, 0);
            std::vector<uint8_t> flags((size_t)(K.w + 2) * (K.h + 2), 0);
            uint8_t cx[J2K_CONTEXTS];
            // an exact-size copy of the block's bytes: a read past them would be seen
            const uint8_t* src = (T.gathered ? gather.data() : streams.data()) + K.off;
            std::vector<uint8_t> bytes(src, src + K.len);
            j2k_block_decode(&K, bytes.data(), v.data(), flags.data(), cx, mq_table);
            for (int y = 0; y < K.h; y++)
                for (int x = 0; x < K.w; x++)
                    coef[K.comp * plane + (size_t)(K.y + y) * tile_w + K.x + x] = j2k_dequant(v[(size_t)y * K.w + x], T.reversible, K.step);
        }
        for (int c = 0; c < 3; c++)
            j2k_idwt(c == 0 ? tile_w : (tile_w + T.dx - 1) / T.dx, tile_h, T.levels, T.reversible, &coef[c * plane], &tmp[c * plane], tile_w, 0, 1, [] {});
        uint8_t* dst = planes.data() + (size_t)tile * 3 * plane;
        for (int y = 0; y < tile_h; y++)
            for (int x = 0; x < tile_w; x++) {
                uint8_t px[3];
                const size_t at = (size_t)y * tile_w;
                j2k_pixel(coef[at + x], coef[plane + at + x / T.dx], coef[2 * plane + at + x / T.dx], T.reversible, T.mct, px);
                for (int c = 0; c < 3; c++) dst[c * plane + at + x] = px[c];
            }
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
    if (argc < 2 || argc > 3) { fprintf(stderr, "usage: %s <directory of .job files> [--hits]\n", argv[0]); return 2; }
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
    if (argc == 3 && std::string(argv[2]) == "--hits") {
        printf("contexts:");
        for (int i = 0; i < 19; i++) printf(" %llu", g_hits[i]);
        printf("\n");
    }
    return failed ? 1 : 0;
}
