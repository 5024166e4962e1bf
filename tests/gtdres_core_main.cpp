// gtdres_core_main.cpp -- gtd::load16_any (vcfgl_amd/csrc/misc/gtdres_core.h: the any-address 16-byte load of k_gtd_bcf_decode under
// --resident 1) as a stand-alone program for the sanitizers (tests/test_gtdres_cli_cpu.py builds it with -fsanitize=address,undefined).
// Every buffer is a heap block of exactly its length, so a piece loaded outside [0, n_bytes) is a report.
//   gtdres_core_main
// For every place `base` 0 .. 15 of the side's first byte behind a 16-byte address, every start residue 0 .. 15 of the 16 bytes asked
// for and every distance 0 .. 40 from their end to the end of the buffer (and starts at the buffer's first bytes): where the loader
// says yes the words are the bytes read one by one; it says yes exactly when the aligned pieces around the bytes lie inside the buffer.
// stdout: "loads <n> joined <n> refused <n>", or "MISMATCH ..." and exit 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "misc/gtdres_core.h"

int main() {
    long loads = 0, joined = 0, refused = 0;
    for (int base = 0; base < 16; base++)
        for (int dist = 0; dist <= 40; dist++)
            for (int64_t o = 0; o < 16 * 6; o++) {
                // the side is `n` bytes that begin `base` bytes into a block of base + n bytes; malloc gives a 16-byte address
                const int64_t n = o + 16 + dist;
                uint8_t* block = (uint8_t*)malloc((size_t)(base + n));
                if (!block || ((uintptr_t)block & 15u) != 0) { printf("MISMATCH the heap gave no 16-byte address\n"); return 1; }
                for (int64_t i = 0; i < base + n; i++) block[i] = (uint8_t)(37 * i + 11 * base + dist + 1);
                const uint8_t* side = block + base;
                uint32_t w[4] = {0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu};
                const bool got = gtd::load16_any(side, o, n, w);
                const int mis = (int)((base + o) & 15);
                const int64_t lo = o - mis;
                const bool want = lo >= 0 && lo + (mis ? 32 : 16) <= n;
                if (got != want) { printf("MISMATCH base %d o %lld dist %d: loader %d, pieces inside %d\n", base, (long long)o, dist, (int)got, (int)want); return 1; }
                if (got) {
                    for (int i = 0; i < 16; i++)
                        if (((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) != side[o + i]) { printf("MISMATCH base %d o %lld dist %d byte %d\n", base, (long long)o, dist, i); return 1; }
                    loads++; joined += mis != 0;
                } else {
                    for (int i = 0; i < 4; i++) if (w[i] != 0xDEADBEEFu) { printf("MISMATCH a refused load wrote its words\n"); return 1; }
                    refused++;
                }
                free(block);
            }
    printf("loads %ld joined %ld refused %ld\n", loads, joined, refused);
    return 0;
}
