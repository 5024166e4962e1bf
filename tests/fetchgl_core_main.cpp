// A host program around vcfgl_amd/csrc/vgl_fetchgl_core.h: the per-value formatter of k_fetchgl_plan / k_fetchgl_write on the CPU,
// where the host sanitizers see every read and write (tests/test_fetchgl_core_cpu.py builds it with -fsanitize=address,undefined and
// runs it).
//   fetchgl_core_main IN OUT
// IN: uint32 float bit patterns.  OUT: for value mode 0 (VGL_FETCHGL_FLOAT), then for value mode 1 (VGL_FETCHGL_TEXT), one line per
// pattern: the value's text and '\n'.
// Every value is formatted twice, as the kernels do: counted without a store, then stored into an allocation of exactly the counted
// size -- a byte written outside it is an AddressSanitizer report, and a second pass that is longer than the first loses its tail
// (the sink never stores at or past its limit), which the comparison against the model then shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vgl_fetchgl_core.h"

namespace fg = vgl_fetchgl;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb"); FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    fseek(fi, 0, SEEK_END);
    const long bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    const size_t n = (size_t)bytes / 4;
    uint32_t* pats = (uint32_t*)malloc(n ? n * 4 : 1);
    if (n && fread(pats, 4, n, fi) != n) { fprintf(stderr, "short input\n"); return 2; }
    uint32_t longest = 0;
    for (int mode = 0; mode < 2; ++mode) {
        for (size_t k = 0; k < n; ++k) {
            fg::Emit<false> c{nullptr, 0, 0};
            fg::fmt_value(c, pats[k], mode);
            if (c.n > longest) longest = c.n;
            uint8_t* buf = (uint8_t*)malloc(c.n ? c.n : 1);
            memset(buf, '#', c.n ? c.n : 1);
            fg::Emit<true> w{buf, 0, c.n};
            fg::fmt_value(w, pats[k], mode);
            if (w.n != c.n) { fprintf(stderr, "pattern %08x mode %d: counted %u, wrote %u\n", pats[k], mode, c.n, w.n); return 1; }
            fwrite(buf, 1, c.n, fo);
            fputc('\n', fo);
            free(buf);
        }
    }
    // the genotype index over every allele table of up to five distinct alleles' first entries and every pair
    long lines = 0;
    for (int nA = 0; nA <= 5; ++nA)
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 5; ++b) {
                int8_t* t = (int8_t*)malloc(nA ? (size_t)nA : 1);                 // exactly nA entries: no read beyond them
                for (int j = 0; j < nA; ++j) t[j] = (int8_t)((j + 1) % 5);
                if (fg::genotype_index(t, nA, a, b) >= 0) lines++;
                free(t);
            }
    printf("values %zu longest %u genotypes %ld\n", n, longest, lines);
    free(pats);
    fclose(fi); fclose(fo);
    return longest <= (uint32_t)fg::MAX_VALUE_LEN ? 0 : 1;
}
