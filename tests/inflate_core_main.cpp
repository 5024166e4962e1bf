// A host program around vcfgl_amd/csrc/vgl_inflate_core.h: the decoder of k_inflate_member on the CPU, where the host sanitizers
// see every read and write (tests/test_inflate_core_cpu.py builds it with -fsanitize=address,undefined and runs it).
//   inflate_core_main IN OUT
// IN:  per member  uint32 size, the member's bytes.   OUT: per member  uint32 status (0 OK, 1 HOST), uint32 check (which check of
// the decoder refused it, 100 header, 101 CRC32), uint32 n, n output bytes (n = ISIZE for status 0, else 0).
// Every member is copied into an allocation of exactly its size and decoded into one of exactly ISIZE bytes: a byte read or
// written outside either is an AddressSanitizer report.  What the kernel does around the decoder is done here the same way: the
// header walk (vgl_bgzf_member_at), ISIZE <= 65536, CRC32 of the output against the trailer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vgl_inflate_core.h"

static uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t r = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        r ^= p[i];
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
    }
    return r ^ 0xffffffffu;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb"); FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    vgl_inflate_tabs* tabs = (vgl_inflate_tabs*)malloc(sizeof(vgl_inflate_tabs));
    uint32_t size;
    long n_members = 0;
    while (fread(&size, 4, 1, fi) == 1) {
        uint8_t* member = (uint8_t*)malloc(size ? size : 1);
        if (size && fread(member, 1, size, fi) != size) { fprintf(stderr, "short input\n"); return 2; }
        int32_t msize = 0, at = 0; uint32_t crc = 0, isize = 0;
        uint32_t rec[3] = {1, 100, 0};
        uint8_t* win = nullptr;
        if (vgl_bgzf_member_at(member, 0, size, msize, at, crc, isize) && (uint32_t)msize == size && isize <= 65536u) {
            win = (uint8_t*)malloc(isize ? isize : 1);
            memset(tabs, 0xa5, sizeof *tabs);                                   // (no table entry may be used before it is built)
            const int rc = vgl_inflate_core(member + at, (int32_t)size - at - 8, win, (int32_t)isize, tabs, 0, 1);
            rec[1] = (uint32_t)rc;
            if (rc == 0) {
                if (crc32_of(win, isize) == crc) { rec[0] = 0; rec[2] = isize; }
                else rec[1] = 101;
            }
        }
        fwrite(rec, 4, 3, fo);
        if (rec[2]) fwrite(win, 1, rec[2], fo);
        free(win); free(member);
        n_members++;
    }
    // the member walk of vgl_bgzf_index over the same bytes laid back to back, in an allocation of exactly their size
    fseek(fi, 0, SEEK_SET);
    size_t total = 0, cap = 1 << 16;
    uint8_t* all = (uint8_t*)malloc(cap);
    while (fread(&size, 4, 1, fi) == 1) {
        if (total + size > cap) { while (total + size > cap) cap *= 2; all = (uint8_t*)realloc(all, cap); }
        if (size && fread(all + total, 1, size, fi) != size) return 2;
        total += size;
    }
    uint8_t* exact = (uint8_t*)malloc(total ? total : 1);
    memcpy(exact, all, total);
    int64_t* begin = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_members + 1));
    int32_t* cs = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_members + 1));
    int32_t* is = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_members + 1));
    int64_t n = -1;
    const int rc = vgl_bgzf_index_core(exact, (int64_t)total, n_members, begin, cs, is, &n);
    int64_t cut = -1;                                                           // and over every prefix cut inside the last member: refused
    int cut_ok = 1;
    if (rc == 0 && n > 0)
        for (int64_t c = begin[n - 1] + 1; c < (int64_t)total; c += 1 + (total - begin[n - 1]) / 64) {
            uint8_t* pre = (uint8_t*)malloc((size_t)c);
            memcpy(pre, exact, (size_t)c);
            if (vgl_bgzf_index_core(pre, c, n_members, begin, cs, is, &cut) == 0) cut_ok = 0;
            free(pre);
        }
    printf("members %ld index %d %lld cut_refused %d\n", n_members, rc, (long long)n, cut_ok);
    free(begin); free(cs); free(is); free(exact); free(all); free(tabs);
    fclose(fi); fclose(fo);
    return 0;
}
