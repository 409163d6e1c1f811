// What the HE2RNA top-k kernels of he2rna.hip and he2rna_train.hip share: the bounds on tiles per slide and values of k, and
// the list of ks as a kernel argument.
#pragma once
#include "sq_common.h"

constexpr int HE_MAX_N = 128, HE_MAX_KS = 16;

struct HeKs {
    int k[HE_MAX_KS];
    int n;
    float scale;
};

static inline int he_fill_ks(const int32_t* ks, int n_ks, float scale, int N, HeKs* o) {
    SQ_REQUIRE(ks && n_ks >= 1 && n_ks <= HE_MAX_KS, "he2rna: %d values of k (1..%d)", n_ks, HE_MAX_KS);
    for (int i = 0; i < n_ks; ++i) {
        SQ_REQUIRE(ks[i] >= 1 && ks[i] <= N, "he2rna: k=%d out of range for %d tiles (torch.topk would raise)", ks[i], N);
        o->k[i] = ks[i];
    }
    o->n = n_ks;
    o->scale = scale;
    return SQ_OK;
}
