// Host build of the XCD tile walk (sequoia-pub_amd/csrc/tile_walk.h) for tests/test_tile_walk_host.py, which compiles this
// stand-alone program with the host compiler and the sanitizers and checks what it prints: for every grid size n on the
// command line one line "n: sq_xcd_tile(0, n) sq_xcd_tile(1, n) ... sq_xcd_tile(n - 1, n)".
#include "../sequoia-pub_amd/csrc/tile_walk.h"

#include <cstdio>
#include <cstdlib>

static_assert(sq_xcd_tile(0, 1) == 0 && sq_xcd_tile(9, 10) == 3, "usable in constant expressions");

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const int n = atoi(argv[i]);
        if (n < 1) { fprintf(stderr, "ERROR: grid size '%s'\n", argv[i]); return 2; }
        printf("%d:", n);
        for (int b = 0; b < n; ++b) printf(" %d", sq_xcd_tile(b, n));
        printf("\n");
    }
    return 0;
}
