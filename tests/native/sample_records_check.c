/* Host build of the per-record function of the sample records (bdpt_math.h bdpt_sample_record,
 * the code bdpt_sample_records_kernel runs on the device), for tests/test_sample_records.py:
 *     sample_records_check <table.f32> <positions.u32> <out.f32>
 * reads the random table (floats) and a list of table positions j (uint32, each j + 4 inside the
 * table) and writes the 8 floats of every position's record.  Build with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_math.h"

static void *slurp(const char *path, size_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    void *p = malloc(n > 0 ? (size_t)n : 1);
    if (p && fread(p, 1, (size_t)n, f) != (size_t)n) { free(p); p = NULL; }
    fclose(f);
    *bytes = (size_t)n;
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    size_t tb = 0, pb = 0;
    float *table = slurp(argv[1], &tb);
    uint32_t *pos = slurp(argv[2], &pb);
    if (!table || !pos) return 3;
    const size_t nt = tb / 4, np = pb / 4;
    static const double tab[BDPT_SC_N][2] = BDPT_SINCOS_TABLE_INIT;
    double sintab[BDPT_SC_N];               /* the device's LDS copy: sin(2pi k/N) only */
    for (int k = 0; k < BDPT_SC_N; k++) sintab[k] = tab[k][0];
    float *out = malloc(np * 8 * sizeof(float) + 1);
    if (!out) return 3;
    for (size_t i = 0; i < np; i++) {
        if ((size_t)pos[i] + 5 > nt) return 4;
        bdpt_sample_record(table + pos[i], sintab, out + 8 * i);
    }
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out, sizeof(float), np * 8, f) != np * 8 || fclose(f) != 0) return 5;
    printf("ok %zu records\n", np);
    return 0;
}
