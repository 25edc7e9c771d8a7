// exact_forms_check.cpp -- exhaustive host check of gym_kilobots_amd/csrc/kb_exact.h (compiled and run by
// tests/test_exact_forms_cpu.py with the system compiler; -ffp-contract=off, the fused multiply-adds are explicit).
//
//   exact_forms_check div K_bits [K_bits ...]     a / K, every mantissa x every exponent of |C| x both signs, and both zeros
//   exact_forms_check rcp ex [ex ...]             1 / x, every mantissa of the binades 2^ex but all ones (see guard) x every seed within 1 ulp
//   exact_forms_check sqrt ex [ex ...]            sqrt(x), every x of the binades inside kb_exact_guard x every pair of seeds (v_sqrt_f32, v_rsq_f32) within 1 ulp
//   exact_forms_check guard ex [ex ...]           no dd inside kb_exact_guard has a sqrtf(dd) with an all-ones mantissa
//   exact_forms_check unguarded ex [ex ...]       rcp and sqrt over EVERY mantissa: what the guard's mantissa clause is there for
//   exact_forms_check rcp_rsq ex [ex ...]         (left out of the kernel: it misses) 1 / sqrtf(x) refined from the seeds of 1 / sqrt(x)
//   exact_forms_check sqrt_rsq ex [ex ...]        (left out of the kernel: it misses) sqrt(x) from s0 = x * y0 alone
//
// One line per case: "<form> <case> checked <n> mismatches <m>"; the exit status is 0 when every m is 0.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "kb_exact.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// every float within one ulp of the exact value v (ulp: the spacing of the floats in v's binade): what an instruction
// documented as "1 ulp" may return
static int seeds(double v, float out[5]) {
    const double ulp = std::ldexp(1.0, std::ilogb(v) - 23);
    float c = (float)v;
    c = std::nextafterf(std::nextafterf(c, 0.0f), 0.0f);
    int n = 0;
    for (int i = 0; i < 5; ++i, c = std::nextafterf(c, INFINITY))
        if (std::fabs((double)c - v) <= ulp) out[n++] = c;
    return n;
}

struct Count { std::atomic<unsigned long long> checked{0}, bad{0}; };

// fn(m, checked, bad) over the 2^23 mantissas, on a few threads
static void over_mantissas(Count &cnt, const std::function<void(uint32_t, unsigned long long &, unsigned long long &)> &fn) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 8 ? 8 : nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            unsigned long long c = 0, b = 0;
            for (uint32_t m = t; m < (1u << 23); m += nt) fn(m, c, b);
            cnt.checked += c; cnt.bad += b;
        });
    for (auto &x : th) x.join();
}

static float binade(int ex, uint32_t m) { return from_bits(((uint32_t)(ex + 127) << 23) | m); }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s div|rcp|sqrt|guard|unguarded|rcp_rsq|sqrt_rsq ARG...\n", argv[0]); return 2; }
    const std::string form = argv[1];
    bool allok = true;
    for (int i = 2; i < argc; ++i) {
        Count cnt;
        if (form == "div") {
            const float K = from_bits((uint32_t)strtoul(argv[i], nullptr, 0));
            const float y = 1.0f / K;
            over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                for (int ex = kb::KB_EXACT_C_EXP_MIN; ex <= kb::KB_EXACT_C_EXP_MAX; ++ex) {
                    const float a = binade(ex, m);
                    b += bits(kb::kb_div_const(a, K, y)) != bits(a / K);
                    b += bits(kb::kb_div_const(-a, K, y)) != bits(-a / K);
                    c += 2;
                }
            });
            for (float z : {0.0f, -0.0f}) { cnt.bad += bits(kb::kb_div_const(z, K, y)) != bits(z / K); cnt.checked += 1; }
        } else {
            const int ex = atoi(argv[i]);
            if (form == "rcp") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m);
                    if (m == 0x7FFFFFu) return;
                    float s[5];
                    const int n = seeds(1.0 / (double)x, s);
                    for (int k = 0; k < n; ++k) b += bits(kb::kb_rcp_refine(x, s[k])) != bits(1.0f / x);
                    c += n;
                });
            } else if (form == "sqrt") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m);
                    if (!kb::kb_exact_guard(x)) return;
                    float s[5], y[5];
                    const int ns = seeds(std::sqrt((double)x), s), ny = seeds(1.0 / std::sqrt((double)x), y);
                    const float want = sqrtf(x);
                    for (int k = 0; k < ns; ++k)
                        for (int l = 0; l < ny; ++l) b += bits(kb::kb_sqrt_refine(x, s[k], y[l])) != bits(want);
                    c += ns * ny;
                });
            } else if (form == "guard") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m);
                    if (!kb::kb_exact_guard(x)) return;
                    b += (bits(sqrtf(x)) & 0x7FFFFFu) == 0x7FFFFFu;
                    c += 1;
                });
            } else if (form == "unguarded") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m);
                    float s[5], y[5];
                    const int nr = seeds(1.0 / (double)x, y);
                    for (int k = 0; k < nr; ++k) b += bits(kb::kb_rcp_refine(x, y[k])) != bits(1.0f / x);
                    const int ns = seeds(std::sqrt((double)x), s), ny = seeds(1.0 / std::sqrt((double)x), y);
                    for (int k = 0; k < ns; ++k)
                        for (int l = 0; l < ny; ++l) b += bits(kb::kb_sqrt_refine(x, s[k], y[l])) != bits(sqrtf(x));
                    c += nr + ns * ny;
                });
            } else if (form == "rcp_rsq") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m), len = sqrtf(x);
                    float y[5];
                    const int ny = seeds(1.0 / std::sqrt((double)x), y);
                    for (int l = 0; l < ny; ++l) b += bits(kb::kb_rcp_refine(len, y[l])) != bits(1.0f / len);
                    c += ny;
                });
            } else if (form == "sqrt_rsq") {
                over_mantissas(cnt, [&](uint32_t m, unsigned long long &c, unsigned long long &b) {
                    const float x = binade(ex, m);
                    float y[5];
                    const int ny = seeds(1.0 / std::sqrt((double)x), y);
                    for (int l = 0; l < ny; ++l) b += bits(kb::kb_sqrt_refine(x, x * y[l], y[l])) != bits(sqrtf(x));
                    c += ny;
                });
            } else { fprintf(stderr, "unknown form %s\n", form.c_str()); return 2; }
        }
        printf("%s %s checked %llu mismatches %llu\n", form.c_str(), argv[i], (unsigned long long)cnt.checked, (unsigned long long)cnt.bad);
        allok = allok && cnt.bad == 0;
    }
    return allok ? 0 : 1;
}
