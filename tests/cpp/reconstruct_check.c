/* Stand-alone driver of the reconstruction host path through the C ABI:
 * RS(6,3) on a host-only coder, every pattern of 1..3 lost units (129) at
 * several shard lengths, each rebuilt unit compared with the original stripe
 * and every other out buffer checked untouched; then the plan call, the error
 * paths and the want subset.  tests/test_reconstruct.py builds and runs it
 * plain; it has its own main so the library's host code can also be checked
 * under a sanitizer by hand (add -fsanitize=address,undefined to the
 * compile line the test uses).
 * Prints "ALL OK <checks>" and exits 0 on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/hdfs_ec_amd.h"

enum { K = 6, M = 3, N = K + M, MAXLEN = 4099 };

static int fails = 0;
#define EXPECT(cond, ...)             \
    do {                              \
        if (!(cond)) {                \
            printf("FAIL: ");         \
            printf(__VA_ARGS__);      \
            printf("\n");             \
            fails++;                  \
        }                             \
    } while (0)

static int popcount(unsigned v) {
    int c = 0;
    for (; v; v &= v - 1) c++;
    return c;
}

int main(void) {
    static const size_t lens[] = {1, 15, 16, 17, 64, 4099};
    hec_coder_t *coder = NULL;
    if (hec_coder_create(K, M, HEC_DEVICE_HOST, &coder) != HEC_OK) {
        printf("FAIL: hec_coder_create\n");
        return 1;
    }
    uint8_t *stripe[K]; /* the data units at the longest length */
    for (int i = 0; i < K; i++) stripe[i] = malloc(MAXLEN);
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < K; i++)
        for (size_t b = 0; b < MAXLEN; b++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            stripe[i][b] = (uint8_t)(x >> 24);
        }
    long checks = 0;
    for (size_t li = 0; li < sizeof(lens) / sizeof(lens[0]); li++) {
        const size_t len = lens[li];
        /* tight buffers of exactly len bytes: an overrun lands outside them */
        uint8_t *in[N], *out[N];
        for (int i = 0; i < N; i++) {
            in[i] = malloc(len);
            out[i] = malloc(len);
        }
        for (int i = 0; i < K; i++) memcpy(in[i], stripe[i], len);
        EXPECT(hec_encode(coder, (const uint8_t *const *)in, len, in + K) == HEC_OK, "encode len %zu", len);
        for (unsigned mask = 1; mask < (1u << N); mask++) {
            if (popcount(mask) > M) continue; /* bit i set = unit i lost */
            const uint8_t *shards[N];
            for (int i = 0; i < N; i++) {
                shards[i] = ((mask >> i) & 1) ? NULL : in[i];
                memset(out[i], 0xA5, len);
            }
            const int rc = hec_reconstruct(coder, shards, len, NULL, out);
            EXPECT(rc == HEC_OK, "len %zu mask %#x rc %d", len, mask, rc);
            for (int i = 0; i < N; i++) {
                if ((mask >> i) & 1) {
                    EXPECT(memcmp(out[i], in[i], len) == 0, "len %zu mask %#x unit %d", len, mask, i);
                } else {
                    int clean = 1;
                    for (size_t b = 0; b < len; b++) clean &= out[i][b] == 0xA5;
                    EXPECT(clean, "len %zu mask %#x: out[%d] of a present unit was written", len, mask, i);
                }
                checks++;
            }
        }
        /* want: units 1 and 8 lost, only 8 asked for */
        {
            const uint8_t *shards[N];
            uint8_t want[N] = {0};
            for (int i = 0; i < N; i++) {
                shards[i] = (i == 1 || i == 8) ? NULL : in[i];
                memset(out[i], 0xA5, len);
            }
            want[8] = 1;
            uint8_t *outs[N] = {0};
            outs[8] = out[8]; /* out[1] may be NULL: not a target */
            EXPECT(hec_reconstruct(coder, shards, len, want, outs) == HEC_OK, "want subset len %zu", len);
            EXPECT(memcmp(out[8], in[8], len) == 0, "want subset: unit 8, len %zu", len);
            EXPECT(out[1][0] == 0xA5, "want subset: unit 1 untouched");
            want[0] = 1; /* present */
            EXPECT(hec_reconstruct(coder, shards, len, want, out) == HEC_ERR_INVALID_ARG, "want on a present unit");
            /* a NULL out at a target */
            outs[8] = NULL;
            want[0] = 0;
            EXPECT(hec_reconstruct(coder, shards, len, want, outs) == HEC_ERR_INVALID_ARG, "NULL out at a target");
            /* 4 lost: nothing written */
            shards[0] = shards[2] = NULL;
            memset(out[8], 0xA5, len);
            EXPECT(hec_reconstruct(coder, shards, len, NULL, out) == HEC_ERR_NOT_ENOUGH_SHARDS, "4 lost");
            for (int i = 0; i < N; i++) EXPECT(out[i][0] == 0xA5 && out[i][len - 1] == 0xA5, "4 lost wrote out[%d]", i);
            checks += 5;
        }
        for (int i = 0; i < N; i++) {
            free(in[i]);
            free(out[i]);
        }
    }
    /* the plan: data rows equal hec_decode_plan's, targets ascending */
    {
        uint8_t present[N] = {1, 0, 1, 1, 1, 1, 1, 0, 1};
        size_t nt = 0, surv[K], targ[M], e = 0, dsurv[K], dmiss[K];
        uint8_t mat[M * K], dmat[K * K];
        EXPECT(hec_reconstruct_plan("rs", K, M, present, NULL, &nt, surv, targ, mat) == HEC_OK, "plan");
        EXPECT(nt == 2 && targ[0] == 1 && targ[1] == 7, "plan targets");
        EXPECT(hec_decode_plan(K, M, present, &e, dsurv, dmiss, dmat) == HEC_OK && e == 1, "decode plan");
        EXPECT(memcmp(surv, dsurv, sizeof(surv)) == 0 && memcmp(mat, dmat, K) == 0, "plan data row");
        checks++;
    }
    for (int i = 0; i < K; i++) free(stripe[i]);
    hec_coder_destroy(coder);
    if (fails) return 1;
    printf("ALL OK %ld\n", checks);
    return 0;
}
