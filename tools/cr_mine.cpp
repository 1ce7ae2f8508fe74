// cr_mine.cpp — mines the hard cases of the cr_* transcendentals (ctl_math.h):
// the float32 inputs at which the host's fp64 library result lies within
// MARGIN fp64 ulps of an fp32 rounding boundary, i.e. at which a second fp64
// library a few ulps away could round to another float.  Stand-alone host
// program (libm + OpenMP, at most 16 threads); driven by
// tools/make_cr_hard_cases.py, which writes tests/golden/cr_hard_cases.json.
//
//   cr_mine one <fn> <lo> <hi>      every finite float32 with bits in [lo, hi)
//   cr_mine pow_srgb                cr_pow(v, (float)(1.0 / 2.4)), every positive finite v  (ctl_image.h)
//   cr_mine pow_burn                cr_pow(burn, 4.0f), every positive finite burn          (ctl_image.h)
//   cr_mine pow_fit <nx> <nt>       cr_pow(1 - sample_x, fit) on an nx x nt grid            (ctl_bsdf.h)
//   cr_mine atan2 <seed> <n>        of n generated unit vectors d: family atan2_env (d.x, -d.z)  (ctl_env.h)
//                                   and family atan2_frame (d.y, d.x)             (ctl_bsdf.h, ctl_math.h)
//
// One line per hard case: family, input bits a, input bits b (0 for one
// argument), fp64 result bits, in hexadecimal, sorted.
//
// Build: g++ -O2 -fopenmp -ffp-contract=off cr_mine.cpp -o cr_mine
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <omp.h>

static const int MARGIN = 16;

static inline float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline uint64_t d_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

// y moved by k fp64 ulps (k steps along the ordered doubles).
static inline double step(double y, int k) {
    int64_t i; memcpy(&i, &y, 8);
    if (i < 0) i = INT64_MIN - i;          // sign-magnitude -> ordered
    i += k;
    if (i < 0) i = INT64_MIN - i;
    double r; memcpy(&r, &i, 8); return r;
}
// The mining rule: the two ends of [y - MARGIN, y + MARGIN] round to different floats.
static inline bool hard(double y) {
    if (!std::isfinite(y)) return false;
    return (float)step(y, -MARGIN) != (float)step(y, +MARGIN);
}

struct Case { uint32_t a, b; uint64_t y; int family; };
static bool operator<(const Case& p, const Case& q) {
    return p.family != q.family ? p.family < q.family : (p.a != q.a ? p.a < q.a : p.b < q.b);
}

typedef double (*fn1)(double);
static fn1 one_argument(const std::string& n) {
    if (n == "sin") return sin;
    if (n == "cos") return cos;
    if (n == "tan") return tan;
    if (n == "acos") return acos;
    if (n == "atan") return atan;
    if (n == "exp") return exp;
    if (n == "log") return log;
    if (n == "log2") return log2;
    return nullptr;
}

// Counter-based generator: splitmix64 of (seed, i).
static inline uint64_t mix(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// A unit vector from three 21-bit fields: a point of the cube [-1, 1]^3 (never
// the origin), normalised in fp32 with IEEE operations only, so numpy restates it.
static inline void unit_vector(uint64_t h, float d[3]) {
    float v[3];
    for (int c = 0; c < 3; c++) v[c] = ((float)((h >> (21 * c)) & 0x1fffffu) + 0.5f) * (1.0f / 1048576.0f) - 1.0f;
    float l = 0.0f; l += v[0] * v[0]; l += v[1] * v[1]; l += v[2] * v[2];
    l = sqrtf(l);
    for (int c = 0; c < 3; c++) d[c] = v[c] / l;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: cr_mine one|pow_srgb|pow_burn|pow_fit|atan2 ...\n"); return 2; }
    const std::string mode = argv[1];
    const int threads = std::min(16, omp_get_max_threads());
    std::vector<std::vector<Case>> found(threads);
    std::string family[2] = {mode, mode};

    if (mode == "one" && argc == 5) {
        family[0] = argv[2];
        const fn1 f = one_argument(family[0]);
        if (!f) { fprintf(stderr, "cr_mine: unknown function %s\n", argv[2]); return 2; }
        const int64_t lo = strtoll(argv[3], nullptr, 0), hi = strtoll(argv[4], nullptr, 0);
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1 << 20)
        for (int64_t u = lo; u < hi; u++) {
            const float x = bits_f((uint32_t)u);
            if (!std::isfinite(x)) continue;
            const double y = f((double)x);
            if (hard(y)) found[omp_get_thread_num()].push_back({(uint32_t)u, 0u, d_bits(y), 0});
        }
    } else if ((mode == "pow_srgb" || mode == "pow_burn") && argc == 2) {
        const float e = mode == "pow_srgb" ? (float)(1.0 / 2.4) : 4.0f;
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1 << 20)
        for (int64_t u = 1; u < 0x7f800000; u++) {
            const double y = pow((double)bits_f((uint32_t)u), (double)e);
            if (hard(y)) found[omp_get_thread_num()].push_back({(uint32_t)u, f_bits(e), d_bits(y), 0});
        }
    } else if (mode == "pow_fit" && argc == 4) {
        const int64_t nx = strtoll(argv[2], nullptr, 0), nt = strtoll(argv[3], nullptr, 0);
        const float pi = 3.14159265358979f;
#pragma omp parallel for num_threads(threads) schedule(dynamic, 16)
        for (int64_t j = 0; j < nt; j++) {
            const float thetaI = 1e-4f + (pi - 1e-4f) * ((float)j / (float)(nt - 1));
            const float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));   // ctl_bsdf.h, mf_sample_visible11
            for (int64_t i = 0; i < nx; i++) {
                const float sample_x = 1e-6f + (1.0f - 1e-6f) * ((float)i / (float)nx);
                const float a = 1 - sample_x;
                const double y = pow((double)a, (double)fit);
                if (hard(y)) found[omp_get_thread_num()].push_back({f_bits(a), f_bits(fit), d_bits(y), 0});
            }
        }
    } else if (mode == "atan2" && argc == 4) {
        family[0] = "atan2_env"; family[1] = "atan2_frame";
        const uint64_t seed = strtoull(argv[2], nullptr, 0);
        const int64_t n = strtoll(argv[3], nullptr, 0);
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1 << 20)
        for (int64_t i = 0; i < n; i++) {
            float d[3];
            unit_vector(mix(seed, (uint64_t)i), d);
            const float pairs[2][2] = {{d[0], -d[2]}, {d[1], d[0]}};   // ctl_env.h (d.x, -d.z); ctl_bsdf.h (wi.y, wi.x)
            for (int p = 0; p < 2; p++) {
                const double y = atan2((double)pairs[p][0], (double)pairs[p][1]);
                if (hard(y)) found[omp_get_thread_num()].push_back({f_bits(pairs[p][0]), f_bits(pairs[p][1]), d_bits(y), p});
            }
        }
    } else {
        fprintf(stderr, "cr_mine: bad arguments\n");
        return 2;
    }

    std::vector<Case> all;
    for (auto& v : found) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end(), [](const Case& p, const Case& q) { return p.family == q.family && p.a == q.a && p.b == q.b; }),
              all.end());
    for (const Case& c : all)
        printf("%s %08x %08x %016llx\n", family[c.family].c_str(), c.a, c.b, (unsigned long long)c.y);
    return 0;
}
