// The arithmetic of oetr_dual_softmax_match on the HOST: imagematching_oetr_amd/csrc/dual_softmax_math.h - the one copy
// the kernels use - compiled as plain C++, with the kernels' walk restated serially (a query's four (key wave, lane
// half) owners as loops, their two accumulators as two registers, the shuffle and the LDS merge as the tree).
// tests/test_dual_softmax_cpu.py loads it and compares e, every statistic, every confidence and every decision with
// the numpy specification bit for bit, so a slip between the specification and the header shows on a machine without
// a GPU.
//
// Build (tools/README.md):  make -C imagematching_oetr_amd/csrc hostmath-dual_softmax
#include <cmath>
#include <cstdint>
#include <stddef.h>
#include <vector>

#include "../imagematching_oetr_amd/csrc/dual_softmax_math.h"

using namespace oetr;

namespace {

constexpr int KT = 128;              // key rows of a tile

// column j of the tile at k0 that register g of accumulator a of lane half h of key wave kh holds
int column(int k0, int kh, int h, int a, int g) { return k0 + kh * 64 + a * 32 + 4 * h + (g & 3) + 8 * (g >> 2); }

float chain(const float* x, const float* y, int D) {
  float acc = 0.0f;
  for (int d = 0; d < D; ++d) acc = fmaf(x[d], y[d], acc);
  return acc;
}

// sweeps 1 and 2 of one direction: Q [Kq][D] asks, K [Kk][D] answers; m, Z [Kq]
void statistics(const float* Q, int Kq, const float* K, int Kk, int D, float scale, float* m, float* Z) {
  for (int i = 0; i < Kq; ++i) {
    float mx[2][2] = {{-INFINITY, -INFINITY}, {-INFINITY, -INFINITY}};
    for (int k0 = 0; k0 < Kk; k0 += KT)
      for (int kh = 0; kh < 2; ++kh)
        for (int h = 0; h < 2; ++h)
          for (int g = 0; g < 16; ++g)
            for (int a = 0; a < 2; ++a) {
              const int j = column(k0, kh, h, a, g);
              if (j < Kk) mx[kh][h] = ds::max_push(mx[kh][h], ds::scaled(chain(Q + (size_t)i * D, K + (size_t)j * D, D), scale));
            }
    const float m0 = mx[0][1] > mx[0][0] ? mx[0][1] : mx[0][0], m1 = mx[1][1] > mx[1][0] ? mx[1][1] : mx[1][0];
    m[i] = m1 > m0 ? m1 : m0;
    float z[2][2][2] = {};
    for (int k0 = 0; k0 < Kk; k0 += KT)
      for (int kh = 0; kh < 2; ++kh)
        for (int h = 0; h < 2; ++h)
          for (int g = 0; g < 16; ++g)
            for (int a = 0; a < 2; ++a) {
              const int j = column(k0, kh, h, a, g);
              if (j >= Kk) continue;
              const float t = ds::scaled(chain(Q + (size_t)i * D, K + (size_t)j * D, D), scale);
              if (ds::finite(t)) z[kh][h][a] = ds::add_term(z[kh][h][a], ds::e(t - m[i]));
            }
    float half[2];
    for (int kh = 0; kh < 2; ++kh)
      half[kh] = ds::tree_node(ds::tree_node(z[kh][0][0], z[kh][0][1]), ds::tree_node(z[kh][1][0], z[kh][1][1]));
    Z[i] = ds::tree_node(half[0], half[1]);
  }
}

// sweep 3 of one direction; conf [Kq][Kk] (or NULL) gets every confidence, -1 where the element is no candidate
void argmax(const float* Q, int Kq, const float* K, int Kk, int D, float scale, const float* m, const float* Z,
            const float* c, const float* Y, float* conf, int32_t* idx, float* val) {
  for (int i = 0; i < Kq; ++i) {
    ds::Best b[2][2] = {{ds::best_empty(), ds::best_empty()}, {ds::best_empty(), ds::best_empty()}};
    for (int k0 = 0; k0 < Kk; k0 += KT)
      for (int kh = 0; kh < 2; ++kh)
        for (int h = 0; h < 2; ++h)
          for (int g = 0; g < 16; ++g)
            for (int a = 0; a < 2; ++a) {
              const int j = column(k0, kh, h, a, g);
              if (j >= Kk) continue;
              const float t = ds::scaled(chain(Q + (size_t)i * D, K + (size_t)j * D, D), scale);
              const float v = ds::confidence(t, m[i], Z[i], c[j], Y[j]);
              if (conf) conf[(size_t)i * Kk + j] = v;
              ds::best_push(b[kh][h], v, j);
            }
    const ds::Best t = ds::best_merge(ds::best_merge(b[0][0], b[0][1]), ds::best_merge(b[1][0], b[1][1]));
    idx[i] = t.i;
    val[i] = t.i >= 0 ? t.v : 0.0f;
  }
}

}  // namespace

extern "C" {

int ds_host_partials(void) { return ds::PARTIALS; }

void ds_host_e(const float* x, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = ds::e(x[i]);
}

void ds_host_slots(int n, int32_t* out) {
  for (int j = 0; j < n; ++j) out[j] = ds::slot(j);
}

// One pair: A [L][D] on an h0 x w0 grid, B [S][D] on h1 x w1.  Outputs: m, Z [L]; c, Y [S]; conf [L][S]; matches0,
// scores0 [L]; matches1 [S]; counts [4].
void ds_host_pair(const float* A, int L, int h0, int w0, const float* B, int S, int h1, int w1, int D, float scale,
                  float threshold, int border, float* m, float* Z, float* c, float* Y, float* conf, int32_t* matches0,
                  float* scores0, int32_t* matches1, int32_t* counts) {
  statistics(A, L, B, S, D, scale, m, Z);
  statistics(B, S, A, L, D, scale, c, Y);
  argmax(A, L, B, S, D, scale, m, Z, c, Y, conf, matches0, scores0);
  std::vector<float> unused(S > 0 ? S : 1);
  argmax(B, S, A, L, D, scale, c, Y, m, Z, nullptr, matches1, unused.data());
  int over = 0, kept = 0;
  for (int i = 0; i < L; ++i) {                                      // k_ds_decide
    const int j = matches0[i];
    bool pass = (unsigned)j < (unsigned)S;
    pass = pass && scores0[i] > threshold && ds::inside(i, h0, w0, border) && ds::inside(j, h1, w1, border);
    const bool keep = pass && matches1[j] == i;
    if (!keep) matches0[i] = -1;
    over += pass, kept += keep;
  }
  counts[0] = L, counts[1] = S, counts[2] = over, counts[3] = kept;
}

}  // extern "C"
