// host_util.h -- what every unit of the front end uses: the fatal-error exit, the clock, split() and the number text of VCF records
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <errno.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/vcfgl_hip.h"
#include "vcf_sink.h"

// Records are parsed, simulated and encoded on several threads, and any of them may hit a fatal input error: the first
// one reports and leaves through _exit() (no static destructors run under the feet of the threads still working, which is
// what exit() from two threads at once did), the others park.
static std::atomic<bool> g_dying{false};
[[noreturn]] static void die_v(const char* fmt, va_list ap) {
    if (g_dying.exchange(true)) for (;;) pause();
    fflush(stdout);
    fprintf(stderr, "\n\n*******\n[ERROR] "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n*******\n");
    fflush(NULL);
    _exit(1);                                  // shared.h:292-299 exit(1)
}
[[noreturn]] static void die(const char* fmt, ...) { va_list ap; va_start(ap, fmt); die_v(fmt, ap); }
[[noreturn]] void vsink::fail(const char* fmt, ...) { va_list ap; va_start(ap, fmt); die_v(fmt, ap); }

static double now_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

// Batches through a handle that holds two at a time (vgl_*_host_*): submit 0; submit 1, retire 0; ...; retire the last
template <typename Submit, typename Retire> static void two_in_flight(int64_t n_batches, Submit submit, Retire retire) {
    for (int64_t b = 0; b < n_batches; b++) { submit(b); if (b > 0) retire(b - 1); }
    if (n_batches > 0) retire(n_batches - 1);
}

// a file's bytes through zlib: plain text, gzip / BGZF, or BCF inside either
static std::vector<uint8_t> read_whole(const std::string& fn) {
    std::vector<uint8_t> raw;
    gzFile fp = gzopen(fn.c_str(), "r");
    if (!fp) die("Could not open file: %s", fn.c_str());
    gzbuffer(fp, 1 << 20);
    std::vector<uint8_t> chunk(1 << 22);
    int k;
    while ((k = gzread(fp, chunk.data(), (unsigned)chunk.size())) > 0) raw.insert(raw.end(), chunk.begin(), chunk.begin() + k);
    gzclose(fp);
    return raw;
}

static void split(const std::string& s, char c, std::vector<std::string>& out) {
    out.clear(); size_t b = 0;
    while (true) { size_t e = s.find(c, b); if (e == std::string::npos) { out.push_back(s.substr(b)); break; } out.push_back(s.substr(b, e - b)); b = e + 1; }
}

// ---------------------------------------------------------------------------------------
// htslib kputd(): floats of VCF text.  0 -> "0"; outside [1e-4, 999999] -> "%g"; otherwise
// trunc(d*1e10) plus half a unit of the 6th significant digit, cut to 6 significant digits,
// trailing zeros removed.
static void put_float(std::string& s, float f) {
    uint32_t bits; memcpy(&bits, &f, 4);
    if (bits == VGL_FLOAT_MISSING_BITS) { s += '.'; return; }
    double d = f;
    if (isnan(d)) { s += "nan"; return; }
    if (d == 0) { s += signbit(d) ? "-0" : "0"; return; }
    if (d < 0) { s += '-'; d = -d; }
    char buf[64];
    if (!(d >= 0.0001 && d <= 999999)) { snprintf(buf, sizeof buf, "%g", d); s += buf; return; }
    uint64_t i = (uint64_t)(d * 10000000000LL);
    if (d < .0001) i += 0; else if (d < 0.001) i += 5; else if (d < 0.01) i += 50; else if (d < 0.1) i += 500;
    else if (d < 1) i += 5000; else if (d < 10) i += 50000; else if (d < 100) i += 500000; else if (d < 1000) i += 5000000;
    else if (d < 10000) i += 50000000; else if (d < 100000) i += 500000000; else i += 5000000000LL;
    char dig[32]; int n = snprintf(dig, sizeof dig, "%llu", (unsigned long long)i);   // d*1e10 as an integer
    std::string out;
    if (n <= 10) {                       // d < 1: "0." + leading zeros + 6 significant digits
        out = "0.";
        out.append(10 - n, '0');
        out.append(dig, n < 6 ? n : 6);
    } else {                             // integer part has n-10 digits; 6 significant digits in all
        const int ip = n - 10;
        out.append(dig, ip);
        if (ip < 6) { out += '.'; out.append(dig + ip, 6 - ip); }
    }
    if (out.find('.') != std::string::npos) {
        while (out.back() == '0') out.pop_back();
        if (out.back() == '.') out.pop_back();
    }
    s += out;
}

static void put_int(std::string& s, int32_t v) {
    if (v == VGL_INT32_MISSING) { s += '.'; return; }
    char buf[16]; snprintf(buf, sizeof buf, "%d", v); s += buf;
}
