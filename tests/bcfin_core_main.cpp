// bcfin_core_main.cpp -- the per-sample rule of the BCF genotype decoder (vcfgl_amd/csrc/vgl_bcfin_core.h) on the CPU, for the host
// sanitizers (tests/test_bcfin_core_cpu.py).  Reads a case set: int32 n_records, int32 n_samples, then per record int32 type, n,
// n_alleles, int8 allele_map[5], int64 slice bytes and the slice.  Every record is decoded from an allocation of exactly its slice
// into an allocation of exactly its row, so that a byte read or written outside either is a sanitizer report.  Prints per record
// "status allelesum row-in-hex" (the row of a handed-back record is unspecified: "-").
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vgl_bcfin_core.h"

template <class T> static T get(FILE* f) {
    T v;
    if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bcfin_core_main CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int32_t R = get<int32_t>(f), N = get<int32_t>(f);
    for (int32_t i = 0; i < R; i++) {
        const int32_t type = get<int32_t>(f), n = get<int32_t>(f), nal = get<int32_t>(f);
        int8_t map[5];
        for (int k = 0; k < 5; k++) map[k] = get<int8_t>(f);
        const int64_t len = get<int64_t>(f);
        uint8_t* slice = (uint8_t*)malloc((size_t)len);
        uint8_t* row = (uint8_t*)malloc((size_t)N);
        if ((len && !slice) || !row) return 2;
        if (len && fread(slice, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "short case file\n"); return 2; }
        // the slice the record describes is what the file holds (else the core would be right to read further)
        const int w = vgl_bcfin::width(type);
        if (w && n >= 1 && (int64_t)N * n * w != len) { fprintf(stderr, "record %d: %lld bytes for %d x %d x %d\n", i, (long long)len, N, n, w); return 2; }
        for (int32_t s = 0; s < N; s++) row[s] = 0xA5;
        int32_t sum = -1;
        const int st = vgl_bcfin::record(slice, type, n, nal, map, N, row, &sum);
        printf("%d ", st);
        if (st == vgl_bcfin::ST_OK) { printf("%d ", sum); for (int32_t s = 0; s < N; s++) printf("%02x", row[s]); } else printf("- -");
        printf("\n");
        free(slice); free(row);
    }
    fclose(f);
    return 0;
}
