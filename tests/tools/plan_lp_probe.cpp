// plan_lp_probe.cpp -- time of the duration planner's cutting planes with the restricted LP of
// small-project-uv-robot-ray-tracer_amd/csrc/uvrt_plan_lp.h on a synthetic covering LP of the planner's shape (host only):
// P candidates on a grid, R rows, counts falling off as 1/d^2, 30 % occluded.  DESIGN.md 9, profiles/r05/r05_lp_probe.txt.
//   g++ -O2 -std=c++17 -ffp-contract=off -I small-project-uv-robot-ray-tracer_amd/csrc tests/tools/plan_lp_probe.cpp -o /tmp/plan_lp_probe
//   /tmp/plan_lp_probe P [R]
#include "uvrt_plan_lp.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <algorithm>
using namespace uvrt_plan_lp;
int main(int argc, char** argv) {
    int P = atoi(argv[1]); int R = argc > 2 ? atoi(argv[2]) : 20000;
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> U(0, 10);
    std::vector<double> px(P), pz(P);
    int side = (int)std::ceil(std::sqrt((double)P));
    for (int p = 0; p < P; ++p) { px[p] = 10.0 * (p % side + 0.5) / side; pz[p] = 10.0 * (p / side + 0.5) / side; }
    std::vector<double> A((size_t)R * P);
    for (int i = 0; i < R; ++i) { double x = U(g), z = U(g); double b = 0.5 + 0.15 * U(g);
        for (int p = 0; p < P; ++p) { double d2 = (x-px[p])*(x-px[p]) + (z-pz[p])*(z-pz[p]) + 1; bool occ = U(g) < 3.0;
            A[(size_t)i*P+p] = occ ? 0 : std::floor(4e3 / d2 * (0.8 + 0.04*U(g))) / (b*1e3); } }
    auto t0 = std::chrono::steady_clock::now();
    RestrictedLP lp(P);
    std::vector<double> d(P, 1.0), ratio(R), y, dd; std::vector<char> inW(R, 0); std::vector<int> W;
    { double mn = 1e300; for (int i = 0; i < R; ++i) { double s = 0; for (int p = 0; p < P; ++p) s += A[(size_t)i*P+p]; mn = std::min(mn, s);} for (auto& v : d) v = 1/mn; }
    int64_t piv = 0; double lb = 0, ub = 1e300; int round = 0;
    for (;; ++round) {
        double mn = 1e300, sd = 0; for (double v : d) sd += v;
        for (int i = 0; i < R; ++i) { double s = 0; for (int p = 0; p < P; ++p) s += A[(size_t)i*P+p]*d[p]; ratio[i] = s; mn = std::min(mn, s); }
        ub = std::min(ub, sd / mn);
        if ((ub - lb) <= 1e-3 * ub) break;
        std::vector<int> cand; for (int i = 0; i < R; ++i) if (!inW[i] && (round == 0 || ratio[i] < 1)) cand.push_back(i);
        if (cand.empty()) break;
        size_t take = std::min(cand.size(), (size_t)std::max(64, 2*P));
        std::partial_sort(cand.begin(), cand.begin()+take, cand.end(), [&](int a, int b){ return ratio[a] < ratio[b] || (ratio[a]==ratio[b] && a<b);});
        cand.resize(take); std::sort(cand.begin(), cand.end());
        std::vector<double> blk; for (int i : cand) { inW[i] = 1; W.push_back(i); blk.insert(blk.end(), &A[(size_t)i*P], &A[(size_t)i*P] + P); }
        lp.add_rows(blk.data(), take);
        bool ok = lp.solve(50 * (lp.rows() + P) + 1000, &piv);
        lp.solution(&y, &d);
        std::vector<double> gcol(P, 0); double sy = 0;
        for (size_t j = 0; j < W.size(); ++j) { if (!y[j]) continue; sy += y[j]; for (int p = 0; p < P; ++p) gcol[p] += A[(size_t)W[j]*P+p]*y[j]; }
        double gm = *std::max_element(gcol.begin(), gcol.end()); if (gm > 0) lb = std::max(lb, sy/gm);
        if (!ok) { printf("cap hit\n"); break; }
    }
    double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("P=%d R=%d rounds=%d W=%zu pivots=%lld gap=%.3g time=%.2fs\n", P, R, round, W.size(), (long long)piv, (ub-lb)/ub, s);
}
