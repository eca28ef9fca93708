// Command-line driver of csrc/closed_loop_log.hpp (tests/test_closed_loop_log_arith.py): the closed-loop log's arithmetic run on the host.
//   sums <file>   the file: "T nx n_err", then n_err lines "a b c" (b < 0: the constant c is subtracted), then T lines of nx states; numbers
//                 as strtod reads them (hexadecimal floats, "nan").  The sums are taken tick by tick, exactly as usv_log_record takes them,
//                 and printed as the 64 bits of each double: "sum c=<channel> abs=<hex> sq=<hex>"
//   pack:<mask>   -> "pack nsel=<n> list=<hex> sel=<j0>,<j1>,.."  the nibble list of a state mask and what log_nibble reads back from it
//   list:<i0>,<i1>,..  -> "list list=<hex> sel=.."  likewise for log_pack_list
#include "closed_loop_log.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace usv;

static uint64_t bits(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static int sums(const char *path)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    int T = 0, nx = 0, n_err = 0;
    if (std::fscanf(f, "%d %d %d", &T, &nx, &n_err) != 3 || T < 0 || nx < 1 || nx > 16 || n_err < 0 || n_err > 4) { std::fclose(f); return 2; }
    int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    double c[4] = {0, 0, 0, 0};
    char tok[64];
    auto number = [&](double *v) {
        if (std::fscanf(f, "%63s", tok) != 1) return false;
        *v = std::strtod(tok, nullptr);
        return true;
    };
    for (int k = 0; k < n_err; k++)
        if (std::fscanf(f, "%d %d", &a[k], &b[k]) != 2 || !number(&c[k]) || a[k] < 0 || a[k] >= nx || b[k] >= nx) { std::fclose(f); return 2; }
    std::vector<double> sa((size_t)n_err, 0.0), sq((size_t)n_err, 0.0), x((size_t)nx);
    for (int t = 0; t < T; t++) {
        for (int j = 0; j < nx; j++)
            if (!number(&x[(size_t)j])) { std::fclose(f); return 2; }
        for (int k = 0; k < n_err; k++)
            log_accumulate(log_error(x[(size_t)a[k]], b[k] >= 0 ? x[(size_t)b[k]] : c[k]), &sa[(size_t)k], &sq[(size_t)k]);
    }
    std::fclose(f);
    for (int k = 0; k < n_err; k++) std::printf("sum c=%d abs=%016" PRIx64 " sq=%016" PRIx64 "\n", k, bits(sa[(size_t)k]), bits(sq[(size_t)k]));
    return 0;
}

static void print_sel(uint64_t list, int n)
{
    std::printf(" list=%016" PRIx64 " sel=", list);
    for (int i = 0; i < n; i++) std::printf(i ? ",%d" : "%d", log_nibble(list, i));
    std::printf("\n");
}

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; k++) {
        const std::string s = argv[k];
        if (s == "sums" && k + 1 < argc) {
            const int rc = sums(argv[++k]);
            if (rc) { std::printf("bad input file\n"); return rc; }
        } else if (s.rfind("pack:", 0) == 0) {
            int n = 0;
            const uint64_t list = log_pack_mask((unsigned)std::strtoul(s.c_str() + 5, nullptr, 0), &n);
            std::printf("pack nsel=%d", n);
            print_sel(list, n);
        } else if (s.rfind("list:", 0) == 0) {
            int idx[16], n = 0;
            for (const char *p = s.c_str() + 5; *p && n < 16;) {
                char *end;
                idx[n++] = (int)std::strtol(p, &end, 10);
                p = *end == ',' ? end + 1 : end;
            }
            std::printf("list");
            print_sel(log_pack_list(idx, n), n);
        } else { std::printf("bad token %s\n", argv[k]); return 2; }
    }
    return 0;
}
