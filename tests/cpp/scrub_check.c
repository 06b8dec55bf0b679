/* Stand-alone driver of the scrub host path through the C ABI: RS(10,4) on a
 * host-only coder at several shard lengths (one crosses the host routine's
 * 64 KiB block), exact-length heap copies so that a read past a unit is a
 * heap overrun: a clean stripe, one flipped bit per unit at the first, the
 * last and the block-edge positions, two corrupt units, then
 * hec_scrub_verdict's four outcomes and the argument checks.
 * tests/test_scrub.py builds and runs it.
 * Prints "ALL OK <checks>" and exits 0 on success. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/hdfs_ec_amd.h"

enum { K = 10, M = 4, N = K + M, MAXLEN = 65536 + 17 };

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

int main(void) {
    static const size_t lens[] = {1, 15, 16, 17, 64, 4099, MAXLEN};
    const uint64_t full = ((uint64_t)1 << N) - 1;
    hec_coder_t *coder = NULL;
    if (hec_coder_create(K, M, HEC_DEVICE_HOST, &coder) != HEC_OK) {
        printf("FAIL: hec_coder_create\n");
        return 1;
    }
    uint8_t *stripe[N]; /* the stripe at the longest length */
    for (int i = 0; i < N; i++) stripe[i] = malloc(MAXLEN);
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < K; i++)
        for (size_t b = 0; b < MAXLEN; b++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            stripe[i][b] = (uint8_t)(x >> 24);
        }
    if (hec_encode(coder, (const uint8_t *const *)stripe, MAXLEN, stripe + K) != HEC_OK) {
        printf("FAIL: hec_encode\n");
        return 1;
    }
    int checks = 0;
    for (size_t li = 0; li < sizeof(lens) / sizeof(lens[0]); li++) {
        const size_t len = lens[li];
        uint8_t *v[N]; /* exact-length copies (parity of a prefix is the prefix of the parity) */
        for (int i = 0; i < N; i++) {
            v[i] = malloc(len);
            memcpy(v[i], stripe[i], len);
        }
        hec_scrub_result_t r = {1, 1};
        EXPECT(hec_scrub(coder, (const uint8_t *const *)v, len, &r) == HEC_OK && r.ruled_out == 0 && r.bad_bytes == 0,
               "clean len %zu", len);
        checks++;
        const size_t pos[] = {0, len - 1, 65535, 65536};
        for (int t = 0; t < N; t++)
            for (int p = 0; p < 4; p++) {
                if (pos[p] >= len) continue;
                v[t][pos[p]] ^= 0x04;
                int unit = -7;
                EXPECT(hec_scrub(coder, (const uint8_t *const *)v, len, &r) == HEC_OK &&
                           r.ruled_out == (full & ~((uint64_t)1 << t)) && r.bad_bytes == 1,
                       "len %zu unit %d pos %zu: %#llx %llu", len, t, pos[p], (unsigned long long)r.ruled_out,
                       (unsigned long long)r.bad_bytes);
                EXPECT(hec_scrub_verdict(r.ruled_out, r.bad_bytes, N, &unit) == HEC_SCRUB_LOCATED && unit == t,
                       "len %zu unit %d: verdict", len, t);
                v[t][pos[p]] ^= 0x04;
                checks++;
            }
        if (len >= 2) { /* two units, two positions */
            v[0][0] ^= 1;
            v[N - 1][len - 1] ^= 1;
            EXPECT(hec_scrub(coder, (const uint8_t *const *)v, len, &r) == HEC_OK && r.ruled_out == full &&
                       r.bad_bytes == 2,
                   "two units len %zu", len);
            checks++;
        }
        for (int i = 0; i < N; i++) free(v[i]);
    }
    { /* verdicts */
        int unit = -7;
        EXPECT(hec_scrub_verdict(0, 0, N, &unit) == HEC_SCRUB_CLEAN && unit == -7, "clean verdict");
        EXPECT(hec_scrub_verdict(full & ~(uint64_t)8, 5, N, &unit) == HEC_SCRUB_LOCATED && unit == 3, "located");
        unit = -7;
        EXPECT(hec_scrub_verdict(full, 2, N, &unit) == HEC_SCRUB_MULTIPLE && unit == -7, "multiple");
        EXPECT(hec_scrub_verdict(full & ~(uint64_t)3, 2, N, &unit) == HEC_SCRUB_AMBIGUOUS && unit == -7, "ambiguous");
        EXPECT(hec_scrub_verdict(0, 1, 6, &unit) == HEC_SCRUB_AMBIGUOUS && unit == -7, "m = 1 is ambiguous");
        EXPECT(hec_scrub_verdict(~(uint64_t)0 >> 1, 1, 64, &unit) == HEC_SCRUB_LOCATED && unit == 63, "64 units");
        EXPECT(hec_scrub_verdict(full & ~(uint64_t)8, 5, N, NULL) == HEC_SCRUB_LOCATED, "NULL unit is allowed");
        EXPECT(hec_scrub_verdict(0, 1, 0, &unit) == HEC_ERR_INVALID_ARG, "0 units");
        EXPECT(hec_scrub_verdict(0, 1, 65, &unit) == HEC_ERR_INVALID_ARG, "65 units");
        checks += 9;
    }
    { /* arguments */
        hec_scrub_result_t r = {7, 7};
        const uint8_t *v[N];
        for (int i = 0; i < N; i++) v[i] = stripe[i];
        EXPECT(hec_scrub(coder, v, 0, &r) == HEC_ERR_INVALID_ARG, "shard_len 0");
        EXPECT(hec_scrub(coder, v, 16, NULL) == HEC_ERR_INVALID_ARG, "NULL out");
        EXPECT(hec_scrub(NULL, v, 16, &r) == HEC_ERR_INVALID_ARG, "NULL coder");
        v[N - 1] = NULL;
        EXPECT(hec_scrub(coder, v, 16, &r) == HEC_ERR_INVALID_ARG, "NULL shard");
        EXPECT(r.ruled_out == 7 && r.bad_bytes == 7, "out untouched on error");
        v[N - 1] = stripe[N - 1];
        EXPECT(hec_scrub_device(coder, v, (const size_t[N]){0}, 16, 1, &r, NULL) == HEC_ERR_DEVICE, "host-only coder");
        checks += 6;
    }
    for (int i = 0; i < N; i++) free(stripe[i]);
    hec_coder_destroy(coder);
    if (fails) return 1;
    printf("ALL OK %d\n", checks);
    return 0;
}
