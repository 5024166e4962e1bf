// set_alleles.h -- --set-alleles FILE: the allele file of the reference's misc/setAlleles, one `REF<TAB>ALT[,ALT...]` line per record
// (1 to 4 ALTs; alleles A, C, G, T and the run's own spelling of the unobserved allele), as the 8-byte target entries of
// vgl_ctx_set_alleles: [count, a0 .. a4 as 0 .. 4 (-1 behind the count), 0, 0].  Line i belongs to the i-th simulated site.
#pragma once

#include "sites.h"

static std::vector<int8_t> read_set_alleles(const Args& a) {
    const char* fn = a.set_alleles_fn.c_str();
    const char* nonref = nonref_name(a);
    FILE* fp = fopen(fn, "r");
    if (!fp) die("Could not open file: %s", fn);
    std::vector<int8_t> table;
    std::string line; long ln = 0; int ch;
    auto code = [&](const std::string& nm) -> int {
        if (nm.size() == 1) { const char* q = strchr("ACGT", nm[0]); if (q && *q) return (int)(q - "ACGT"); }
        if (nm == nonref) return 4;
        if (nm == "<*>" || nm == "<NON_REF>")
            die("--set-alleles %s, line %ld: the unobserved allele of this run is spelled %s (-doUnobserved %d), not %s.", fn, ln, nonref, a.do_unobserved, nm.c_str());
        die("--set-alleles %s, line %ld: unknown allele '%s' (A, C, G, T or %s).", fn, ln, nm.c_str(), nonref);
        return -1;
    };
    auto take = [&]() {
        ln++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 >= line.size() || line.find('\t', tab + 1) != std::string::npos)
            die("--set-alleles %s, line %ld: expected REF<TAB>ALT[,ALT...], found '%s'.", fn, ln, line.c_str());
        std::vector<std::string> names{line.substr(0, tab)};
        for (size_t b = tab + 1;;) {
            const size_t e = line.find(',', b);
            names.push_back(line.substr(b, e == std::string::npos ? e : e - b));
            if (names.back().empty()) die("--set-alleles %s, line %ld: an empty ALT allele in '%s'.", fn, ln, line.c_str());
            if (e == std::string::npos) break;
            b = e + 1;
        }
        if (names.size() > 5) die("--set-alleles %s, line %ld: %zu ALT alleles; at most 4 are supported.", fn, ln, names.size() - 1);
        int8_t e8[8] = {(int8_t)names.size(), -1, -1, -1, -1, -1, 0, 0};
        for (size_t j = 0; j < names.size(); j++) {
            const int c = code(names[j]);
            for (size_t k = 0; k < j; k++) if (e8[1 + k] == c) die("--set-alleles %s, line %ld: allele %s is named twice.", fn, ln, names[j].c_str());
            e8[1 + j] = (int8_t)c;
        }
        table.insert(table.end(), e8, e8 + 8);
        line.clear();
    };
    while ((ch = fgetc(fp)) != EOF) { if (ch == '\n') take(); else line += (char)ch; }
    if (!line.empty()) take();
    fclose(fp);
    return table;
}
