// jg_dc_island.cpp -- host only: which buses leave with a bridge of the DC N-1 screen (jg_dc.hpp has the identity the lanes are solved by).
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/jgrid.h"
#include "jg_dc.hpp"
#include "jg_engine.hpp"

namespace jg {

void dc_island_table(int n, int nbr, const int* from, const int* to, const double* admittance, int slack, int* preorder, int* lo, int* hi, int* side) {
    std::vector<int> ptr(n + 1, 0);
    auto live = [&](int k) { return admittance[k] != 0.0 && from[k] != to[k]; };
    for (int k = 0; k < nbr; ++k)
        if (live(k)) { ptr[from[k] + 1]++; ptr[to[k] + 1]++; }
    for (int i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    std::vector<int> nb(ptr[n]), ed(ptr[n]), fill(ptr.begin(), ptr.end() - 1);
    for (int k = 0; k < nbr; ++k)
        if (live(k)) {
            nb[fill[from[k]]] = to[k]; ed[fill[from[k]]++] = k;
            nb[fill[to[k]]] = from[k]; ed[fill[to[k]]++] = k;
        }
    for (int i = 0; i < n; ++i) preorder[i] = -1;
    for (int k = 0; k < nbr; ++k) { lo[k] = 1; hi[k] = 0; side[k] = 0; }
    std::vector<int> low(n, 0), next(ptr.begin(), ptr.end() - 1), pedge(n, -1), stack;
    int timer = 0;
    preorder[slack] = low[slack] = timer++;
    stack.push_back(slack);
    while (!stack.empty()) {
        const int v = stack.back();
        if (next[v] < ptr[v + 1]) {
            const int u = nb[next[v]], e = ed[next[v]];
            ++next[v];
            if (e == pedge[v]) continue;                                 // the edge v was reached by; a parallel branch has another index and counts
            if (preorder[u] < 0) {
                preorder[u] = low[u] = timer++;
                pedge[u] = e;
                stack.push_back(u);
            } else if (preorder[u] < low[v]) low[v] = preorder[u];
            continue;
        }
        stack.pop_back();
        if (stack.empty()) break;
        const int p = stack.back(), e = pedge[v];
        if (low[v] < low[p]) low[p] = low[v];
        if (low[v] > preorder[p]) {                                      // nothing below v reaches p or above but e itself
            lo[e] = preorder[v]; hi[e] = timer - 1;                      // v's subtree: everything numbered since v
            side[e] = from[e] == p ? 1 : -1;
        }
    }
}

}  // namespace jg

extern "C" int jg_dc_island_table(int64_t n, int64_t nbr, const int64_t* from, const int64_t* to, const double* admittance, int64_t slack,
                                  int32_t* preorder, int32_t* lo, int32_t* hi, int32_t* side) {
    auto fail = [](const char* msg) { jg::set_last_error(std::string("jg_dc_island_table: ") + msg); return 1; };
    if (n < 1 || n > (1 << 24) || nbr < 0 || nbr > (1 << 26) || slack < 1 || slack > n || !preorder || (nbr && (!from || !to || !admittance || !lo || !hi || !side)))
        return fail("bad argument");
    std::vector<int> f(nbr), t(nbr);
    for (int64_t k = 0; k < nbr; ++k) {
        if (from[k] < 1 || from[k] > n || to[k] < 1 || to[k] > n) return fail("bus index out of range");
        f[k] = (int)from[k] - 1; t[k] = (int)to[k] - 1;
    }
    static_assert(sizeof(int) == sizeof(int32_t), "int is 32 bits");
    jg::dc_island_table((int)n, (int)nbr, f.data(), t.data(), admittance, (int)slack - 1, preorder, lo, hi, side);
    return 0;
}
