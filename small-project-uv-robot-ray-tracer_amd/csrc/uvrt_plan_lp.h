// uvrt_plan_lp.h -- the restricted LP of the duration planner's cutting planes (host code, no HIP; uvrt_plan.hip)
//
// Over the rows W gathered so far the planner needs the covering LP  min 1.d  s.t.  A_W d >= 1, d >= 0  and a dual
// certificate.  RestrictedLP solves its dual  max 1.y  s.t.  A_W^T y <= 1 + delta, y >= 0  (P constraints, one column
// per row of W) by a tableau simplex:
//   * the slack basis is feasible from the start, and rows added in a later round are new COLUMNS of this dual, so the
//     previous optimal basis stays feasible: every round after the first warm-starts from it (new columns are priced
//     through B^-1, which the tableau's slack block holds);
//   * Dantzig pricing (most negative reduced cost, lowest index on ties); ratio test ties go to the largest pivot;
//   * the right-hand side is perturbed, 1 + delta_p with delta_p in [1e-9, 2e-9), a deterministic function of p, so the
//     covering LP's massive degeneracy (many rows tie at the optimum) does not stall the pivots.  The perturbation
//     does not weaken anything: y stays a valid certificate (the caller divides sum y by max_p (A^T y)_p) and d = the
//     shadow prices covers every row of W (A_W d >= 1 holds for the dual of any right-hand side).
//   * a pivot candidate must exceed 1e-12 x the largest |entry| of the ENTERING COLUMN.  The floor is relative to that
//     column alone, not to the largest entry of the whole matrix: the rows are scaled by r_t (and, bounded, by 1 / rho_t
//     with rho_t down to 1e-9), so entries of different rows may lie more than 1e12 apart, and a floor taken from the
//     largest of them would hide the only positive entry of a small row's column and call a covering LP unbounded.
// d_p is the objective row's entry under slack p: exactly 0 for a position whose constraint is slack.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace uvrt_plan_lp {

class RestrictedLP {
public:
    explicit RestrictedLP(int P) : P_(P), cap_(0), n_(0), rhs_((size_t)P + 1, 0.0), basis_(P), col_((size_t)P, 0.0)
    {
        grow(std::max(64, 2 * P));
        for (int p = 0; p < P; ++p) {
            at(p, p) = 1.0;
            const uint32_t h = (uint32_t)p * 2654435761u;
            rhs_[p] = 1.0 + 1e-9 * (1.0 + (double)(h >> 8) / 16777216.0);
            basis_[p] = p;
        }
    }
    int64_t rows() const { return n_; }

    // append rows of A_W (k x P, row-major) as columns of the dual, priced against the current basis
    void add_rows(const double* a, int64_t k)
    {
        if (P_ + n_ + k > cap_) grow(std::max(P_ + n_ + k, 2 * cap_));
        for (int64_t j = 0; j < k; ++j) {
            const double* aj = a + (size_t)j * P_;
            const int64_t col = P_ + n_ + j;
            for (int q = 0; q < P_; ++q) {           // B^-1 a_j: the slack block of row q is row q of B^-1
                const double* bq = &at(q, 0);
                double v = 0.0;
                for (int p = 0; p < P_; ++p) v += bq[p] * aj[p];
                at(q, col) = v;
            }
            double rc = -1.0;                        // reduced cost -1 + d . a_j
            for (int p = 0; p < P_; ++p) rc += at(P_, p) * aj[p];
            at(P_, col) = rc;
        }
        n_ += k;
    }

    // pivots until optimal (true) or max_pivots (false: the last basis is still feasible)
    bool solve(int64_t max_pivots, int64_t* pivots)
    {
        const int64_t cols = P_ + n_;
        for (int64_t it = 0;; ++it) {
            int64_t e = -1;
            double best = -1e-12;
            const double* obj = &at(P_, 0);
            for (int64_t k = 0; k < cols; ++k)
                if (obj[k] < best) { best = obj[k]; e = k; }
            if (e < 0) { if (pivots) *pivots += it; return true; }
            if (it >= max_pivots) { if (pivots) *pivots += it; return false; }
            double amax = 0.0;                       // the pivot floor is relative to the entering column (above);
            for (int q = 0; q < P_; ++q) {           // one strided walk down the tableau: the column is kept for the ratio test
                col_[q] = at(q, e);
                amax = std::max(amax, std::fabs(col_[q]));
            }
            const double eps = 1e-12 * amax;
            int r = -1;
            double rbest = 0, pbest = 0;
            for (int q = 0; q < P_; ++q) {
                const double a = col_[q];
                if (a <= eps) continue;
                const double ratio = rhs_[q] / a;
                if (r < 0 || ratio < rbest || (ratio == rbest && a > pbest)) { r = q; rbest = ratio; pbest = a; }
            }
            if (r < 0) { if (pivots) *pivots += it; return false; }     // unbounded: not for a covering LP
            pivot(r, e, cols);
        }
    }

    // y per row of W (in the order added) and d per position
    void solution(std::vector<double>* y, std::vector<double>* d) const
    {
        y->assign((size_t)n_, 0.0);
        for (int q = 0; q < P_; ++q)
            if (basis_[q] >= P_) (*y)[basis_[q] - P_] = std::max(0.0, rhs_[q]);
        d->assign(P_, 0.0);
        for (int p = 0; p < P_; ++p) (*d)[p] = std::max(0.0, at(P_, p));
    }

private:
    int P_;
    int64_t cap_, n_;
    std::vector<double> tab_;           // (P + 1) rows x cap_ columns: [slacks | y columns], row P = objective
    std::vector<double> rhs_;           // P + 1
    std::vector<int64_t> basis_;
    std::vector<double> col_;           // P: the entering column of the pivot at hand
    double& at(int64_t q, int64_t k) { return tab_[(size_t)q * cap_ + k]; }
    double at(int64_t q, int64_t k) const { return tab_[(size_t)q * cap_ + k]; }

    void grow(int64_t cap)
    {
        std::vector<double> t((size_t)(P_ + 1) * cap, 0.0);
        for (int q = 0; q <= P_; ++q)
            for (int64_t k = 0; k < P_ + n_; ++k) t[(size_t)q * cap + k] = tab_.empty() ? 0.0 : tab_[(size_t)q * cap_ + k];
        tab_.swap(t);
        cap_ = cap;
    }

    void pivot(int r, int64_t e, int64_t cols)
    {
        double* pr = &at(r, 0);
        const double piv = pr[e];
        for (int64_t k = 0; k < cols; ++k) pr[k] /= piv;
        pr[e] = 1.0;
        rhs_[r] /= piv;
        for (int q = 0; q <= P_; ++q) {
            if (q == r) continue;
            double* pq = &at(q, 0);
            const double f = pq[e];
            if (f == 0.0) continue;
            for (int64_t k = 0; k < cols; ++k) pq[k] -= f * pr[k];
            pq[e] = 0.0;
            rhs_[q] -= f * rhs_[r];
        }
        basis_[r] = e;
    }
};

}  // namespace uvrt_plan_lp
