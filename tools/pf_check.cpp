// pf_check.cpp -- the power-flow equations of csrc/jg_pf.hpp (what the assembling kernels call) checked on the host.
//
// Grids the program makes itself (fixed seed): complete grids of 3 .. 6 buses under EVERY mix of PQ / PV / slack, a grid with a bus that has nothing but
// its diagonal entry (a row of one), and a hub with 18 neighbours (a row of 19 entries, the longest the assembly expects).  On each
//   * the mismatch and the padded Jacobian are formed row by row through the header, the way k_assemble does (mask bits by the host's rule), then
//     f against V conj(Y V) - S in std::complex<double> (1e-12 of the row's scale: at most 19 terms of size O(1) round differently), every existing entry
//     of J against a central difference of that restatement (step 1e-6, 1e-7 of the row's scale), every masked entry == 0, every identity row == identity;
//   * the edit patch: patched<MP> on (g, b) then the formulas == the formulas on (g + dg, b + db), bit for bit;
//   * the dG, dB form of k_comp_fix (the same functions on the edits, identity rows contributing 0) == the difference of two full assemblies (1e-12);
//   * both ends of a branch against I = Y_branch V, S = V conj(I) in complex arithmetic (1e-12).
// Built by tests/test_pf_equations_cpu.py with g++ -fsanitize=address,undefined; exit status 0 = all of it holds.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "../juliagrid.jl_amd/csrc/jg_pf.hpp"

namespace pf = jg::pf;
using cd = std::complex<double>;

struct Entry { int j; double g, b; };
struct Grid {
    int n;
    std::vector<std::vector<Entry>> row;     // Ybus by rows, the diagonal entry among them
    std::vector<int> type;                   // 1 PQ, 2 PV, 3 slack
    std::vector<double> vm, va, p, q;
};
struct Assembled { std::vector<double> J, f, scale; };       // J dense [2n][2n]: block (i, j) at rows 2i, 2i + 1 (P, Q), columns 2j, 2j + 1 (theta, V)

static std::mt19937_64 rng(20240611);
static double uni(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); }
static int failures = 0;
static long long checks = 0;
static void expect(bool ok, const char* what, int a, int b, double got, double want) {
    ++checks;
    if (!ok && ++failures <= 20) std::fprintf(stderr, "pf_check: %s at (%d, %d): got %.17g, want %.17g\n", what, a, b, got, want);
}

// the existence bits of entry (i, j) by the host's rule: rows P unless slack, Q for PQ; columns theta unless slack, V for PQ
static int mask(int ti, int tj) {
    const int rpm = ti != 3, rq = ti == 1, ct = tj != 3, cv = tj == 1;
    return (rpm & ct) | ((rpm & cv) << 1) | ((rq & ct) << 2) | ((rq & cv) << 3);
}

// One pass over the rows, as k_assemble walks them.  one = 1: the padded Jacobian and the mismatch; one = 0 with p = q = 0: what the entries of `g`
// contribute to a DIFFERENCE of two assemblies (k_comp_fix walks the edits of a scenario this way).
static Assembled assemble(const Grid& g, double one) {
    const int n = g.n;
    Assembled a{std::vector<double>(4 * (size_t)n * n, 0.0), std::vector<double>(2 * (size_t)n, 0.0), std::vector<double>((size_t)n, 0.0)};
    auto put = [&](int i, int j, const jg::Blk& b) {
        double* r0 = &a.J[(size_t)(2 * i) * 2 * n + 2 * j];
        double* r1 = r0 + 2 * n;
        r0[0] += b.v00; r0[1] += b.v01; r1[0] += b.v10; r1[1] += b.v11;
    };
    for (int i = 0; i < n; ++i) {
        const double vi = g.vm[i];
        double s1 = 0.0, s2 = 0.0, gii = 0.0, bii = 0.0, scale = std::fabs(g.p[i]) + std::fabs(g.q[i]);
        for (const Entry& e : g.row[i]) {
            const double vj = g.vm[e.j], s = std::sin(g.va[i] - g.va[e.j]), c = std::cos(g.va[i] - g.va[e.j]);
            const pf::Terms t = pf::entry_terms(e.g, e.b, s, c);
            s1 += vj * t.ac;
            s2 += vj * t.ad;
            scale += vi * vj * std::hypot(e.g, e.b);
            if (e.j == i) { gii = e.g; bii = e.b; continue; }
            put(i, e.j, pf::offdiag(mask(g.type[i], g.type[e.j]), vi, vj, t.ac, t.ad));
        }
        const pf::Row r = pf::pad(g.type[i], one, pf::row_closure(vi, s1, s2, gii, bii, g.p[i], g.q[i]));
        put(i, i, r.d);
        a.f[2 * i] = r.fp; a.f[2 * i + 1] = r.fq;
        a.scale[i] = std::max(scale, 1.0);
    }
    return a;
}

// V conj(Y V) - S, the complex restatement
static std::vector<double> mismatch_complex(const Grid& g, const std::vector<double>& vm, const std::vector<double>& va) {
    std::vector<double> f(2 * (size_t)g.n);
    for (int i = 0; i < g.n; ++i) {
        cd cur = 0.0;
        for (const Entry& e : g.row[i]) cur += cd(e.g, e.b) * std::polar(vm[e.j], va[e.j]);
        const cd s = std::polar(vm[i], va[i]) * std::conj(cur) - cd(g.p[i], g.q[i]);
        f[2 * i] = s.real(); f[2 * i + 1] = s.imag();
    }
    return f;
}

static void check_grid(const Grid& g) {
    const int n = g.n;
    const Assembled a = assemble(g, 1.0);
    const std::vector<double> f = mismatch_complex(g, g.vm, g.va);
    auto row_exists = [&](int r) { const int t = g.type[r >> 1]; return (r & 1) ? t == 1 : t != 3; };     // and the column of the same index
    std::vector<char> pattern((size_t)n * n, 0);
    for (int i = 0; i < n; ++i) for (const Entry& e : g.row[i]) pattern[(size_t)i * n + e.j] = 1;
    for (int r = 0; r < 2 * n; ++r) {
        const double want = row_exists(r) ? f[r] : 0.0;
        if (row_exists(r)) expect(std::fabs(a.f[r] - want) <= 1e-12 * a.scale[r >> 1], "mismatch", r, 0, a.f[r], want);
        else expect(a.f[r] == 0.0, "mismatch of an identity row", r, 0, a.f[r], 0.0);
    }
    const double h = 1e-6;
    for (int c = 0; c < 2 * n; ++c) {
        std::vector<double> vm = g.vm, va = g.va;
        double& x = (c & 1) ? vm[c >> 1] : va[c >> 1];
        const double x0 = x;
        x = x0 + h; const std::vector<double> fp = mismatch_complex(g, vm, va);
        x = x0 - h; const std::vector<double> fm = mismatch_complex(g, vm, va);
        for (int r = 0; r < 2 * n; ++r) {
            const double got = a.J[(size_t)r * 2 * n + c];
            if (row_exists(r) && row_exists(c) && pattern[(size_t)(r >> 1) * n + (c >> 1)]) {
                const double want = (fp[r] - fm[r]) / (2.0 * h);
                expect(std::fabs(got - want) <= 1e-7 * a.scale[r >> 1], "Jacobian entry", r, c, got, want);
            } else {
                const double want = r == c ? 1.0 : 0.0;              // masked entries, identity rows and columns: exact
                expect(got == want, "masked / identity entry", r, c, got, want);
            }
        }
    }
}

// J(Y + dY) - J(Y) and f(Y + dY) - f(Y) against the same functions on dY alone with identity rows contributing 0
static void check_comp(const Grid& g) {
    Grid d = g, s = g;
    for (int i = 0; i < g.n; ++i) {
        d.p[i] = d.q[i] = 0.0;
        for (size_t k = 0; k < g.row[i].size(); ++k) {
            const bool edit = uni(0.0, 1.0) < 0.5;
            d.row[i][k].g = edit ? uni(-2.0, 2.0) : 0.0; d.row[i][k].b = edit ? uni(-2.0, 2.0) : 0.0;
            s.row[i][k].g += d.row[i][k].g; s.row[i][k].b += d.row[i][k].b;
        }
    }
    const Assembled a0 = assemble(g, 1.0), a1 = assemble(s, 1.0), m = assemble(d, 0.0);
    for (int r = 0; r < 2 * g.n; ++r) {
        const double tol = 1e-12 * std::max(a0.scale[r >> 1], a1.scale[r >> 1]);
        expect(std::fabs(m.f[r] - (a1.f[r] - a0.f[r])) <= tol, "dG, dB form: mismatch", r, 0, m.f[r], a1.f[r] - a0.f[r]);
        for (int c = 0; c < 2 * g.n; ++c) {
            const size_t k = (size_t)r * 2 * g.n + c;
            expect(std::fabs(m.J[k] - (a1.J[k] - a0.J[k])) <= tol, "dG, dB form: Jacobian", r, c, m.J[k], a1.J[k] - a0.J[k]);
        }
    }
}

static void check_patch() {
    constexpr int MP = 8;
    const size_t ld = 3, b = 1;
    double pdg[MP * 3], pdb[MP * 3];
    for (double& x : pdg) x = uni(-3.0, 3.0);
    for (double& x : pdb) x = uni(-3.0, 3.0);
    const int ppos[MP] = {7, -1, 12, 7, -1, 3, -1, -1};            // entry 7 is edited twice, 12 and 3 once, the others not at all
    for (int p : {3, 7, 12, 5}) {
        const double g0 = uni(-5.0, 5.0), b0 = uni(-5.0, 5.0);
        double g = g0, bb = b0, gs = g0, bs = b0;
        pf::patched<MP>(p, ppos, pdg, pdb, ld, b, g, bb);
        for (int m = 0; m < MP; ++m) if (ppos[m] == p) { gs += pdg[m * ld + b]; bs += pdb[m * ld + b]; }
        expect(g == gs && bb == bs && ((p == 5) == (g == g0 && bb == b0)), "patched entry", p, 0, g, gs);
        const double vi = uni(0.9, 1.1), vj = uni(0.9, 1.1), th = uni(-1.0, 1.0);
        const pf::Terms t = pf::entry_terms(g, bb, std::sin(th), std::cos(th)), ts = pf::entry_terms(gs, bs, std::sin(th), std::cos(th));
        const jg::Blk o = pf::offdiag(15, vi, vj, t.ac, t.ad), os = pf::offdiag(15, vi, vj, ts.ac, ts.ad);
        expect(o.v00 == os.v00 && o.v01 == os.v01 && o.v10 == os.v10 && o.v11 == os.v11, "block of a patched entry", p, 0, o.v00, os.v00);
    }
    double g = 1.5, bb = -2.5;
    pf::patched<0>(7, ppos, pdg, pdb, ld, b, g, bb);
    expect(g == 1.5 && bb == -2.5, "patched<0>", 7, 0, g, 1.5);
}

static void check_branch_ends() {
    for (int t = 0; t < 200; ++t) {
        pf::TwoPort y;
        for (double& x : y.y) x = uni(-10.0, 10.0);
        const double Vi = uni(0.8, 1.2), Vj = uni(0.8, 1.2), ti = uni(-3.0, 3.0), tj = uni(-3.0, 3.0);
        const pf::BranchEnds e = pf::branch_ends(y, Vi, Vj, std::sin(ti), std::cos(ti), std::sin(tj), std::cos(tj));
        const cd vi = std::polar(Vi, ti), vj = std::polar(Vj, tj);
        const cd If = cd(y.y[0], y.y[1]) * vi + cd(y.y[2], y.y[3]) * vj, It = cd(y.y[4], y.y[5]) * vi + cd(y.y[6], y.y[7]) * vj;
        const cd Sf = vi * std::conj(If), St = vj * std::conj(It);
        const double got[8] = {e.ifr, e.ifi, e.itr, e.iti, e.pf, e.qf, e.pt, e.qt};
        const double want[8] = {If.real(), If.imag(), It.real(), It.imag(), Sf.real(), Sf.imag(), St.real(), St.imag()};
        const double scale = std::max(1.0, std::max(std::abs(If), std::abs(It)) * std::max(Vi, Vj) * 4.0);
        for (int k = 0; k < 8; ++k) expect(std::fabs(got[k] - want[k]) <= 1e-12 * scale, "branch end", t, k, got[k], want[k]);
    }
}

// a grid over the given pattern (the diagonal is added): random admittances, a random state, random injections
static Grid make_grid(int n, const std::vector<std::pair<int, int>>& lines) {
    Grid g;
    g.n = n;
    g.row.assign(n, {});
    for (int i = 0; i < n; ++i) g.row[i].push_back(Entry{i, uni(0.5, 8.0), uni(-20.0, -1.0)});
    for (const auto& l : lines) {
        g.row[l.first].push_back(Entry{l.second, uni(-4.0, 0.0), uni(0.5, 10.0)});
        g.row[l.second].push_back(Entry{l.first, uni(-4.0, 0.0), uni(0.5, 10.0)});      // (a phase shifter makes Ybus unsymmetric: nothing here relies on symmetry)
    }
    for (auto& r : g.row) std::shuffle(r.begin(), r.end(), rng);                          // the diagonal entry anywhere in its row
    g.type.assign(n, 1);
    for (int i = 0; i < n; ++i) { g.vm.push_back(uni(0.9, 1.1)); g.va.push_back(uni(-0.6, 0.6)); g.p.push_back(uni(-2.0, 2.0)); g.q.push_back(uni(-1.0, 1.0)); }
    return g;
}

int main() {
    int grids = 0;
    for (int n = 3; n <= 6; ++n) {                                    // complete grids under every mix of bus types
        std::vector<std::pair<int, int>> all;
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) all.push_back({i, j});
        Grid g = make_grid(n, all);
        int mixes = 1;
        for (int i = 0; i < n; ++i) mixes *= 3;
        for (int m = 0; m < mixes; ++m) {
            for (int i = 0, x = m; i < n; ++i, x /= 3) g.type[i] = 1 + x % 3;
            check_grid(g);
            if (m % 7 == 0) check_comp(g);
            ++grids;
        }
    }
    {   // bus 2 has nothing but its diagonal entry: a row of one
        Grid g = make_grid(4, {{0, 1}, {1, 3}, {0, 3}});
        for (int t = 1; t <= 3; ++t) { g.type = {3, 1, t, 2}; check_grid(g); check_comp(g); ++grids; }
    }
    {   // a hub with 18 neighbours: a row of 19 entries
        std::vector<std::pair<int, int>> star;
        for (int j = 1; j <= 18; ++j) star.push_back({0, j});
        Grid g = make_grid(19, star);
        if (g.row[0].size() != 19) { std::fprintf(stderr, "pf_check: the hub's row has %zu entries\n", g.row[0].size()); return 2; }
        for (int t = 1; t <= 3; ++t)
            for (int rep = 0; rep < 4; ++rep) {
                for (int i = 1; i < 19; ++i) g.type[i] = 1 + (int)(rng() % 3);
                g.type[0] = t;
                check_grid(g); check_comp(g); ++grids;
            }
    }
    check_patch();
    check_branch_ends();
    std::printf("pf_check: %d grids, %lld checks, %d failures\n", grids, checks, failures);
    return failures ? 1 : 0;
}
