// xa_tables.cpp -- host builder (fp64) of the XA decimation stage's tables (XaTab,
// zfft_internal.h; kernels xa_kernels.hip, design model tools/xa_proto.py).
#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

#include "cheby1_q2.h"
#include "zfft_internal.h"

namespace zfft {
namespace {

// ---- 8x8 helpers (fp64) for the modal bases of the XA cascades ----
using Mat8 = std::vector<double>;  // 8x8 row-major
Mat8 matmul8(const Mat8 &a, const Mat8 &b) {
  Mat8 c(64, 0.0);
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 8; ++k)
      for (int j = 0; j < 8; ++j) c[i * 8 + j] += a[i * 8 + k] * b[k * 8 + j];
  return c;
}
using cd = std::complex<double>;

void mat_inverse8(const Mat8 &a, Mat8 &inv) {
  Mat8 m = a;
  inv.assign(64, 0.0);
  for (int i = 0; i < 8; ++i) inv[i * 8 + i] = 1.0;
  for (int c = 0; c < 8; ++c) {
    int piv = c;
    for (int r = c + 1; r < 8; ++r)
      if (std::fabs(m[r * 8 + c]) > std::fabs(m[piv * 8 + c])) piv = r;
    for (int k = 0; k < 8; ++k) {
      std::swap(m[c * 8 + k], m[piv * 8 + k]);
      std::swap(inv[c * 8 + k], inv[piv * 8 + k]);
    }
    const double d = m[c * 8 + c];
    for (int k = 0; k < 8; ++k) {
      m[c * 8 + k] /= d;
      inv[c * 8 + k] /= d;
    }
    for (int r = 0; r < 8; ++r) {
      if (r == c) continue;
      const double f = m[r * 8 + c];
      for (int k = 0; k < 8; ++k) {
        m[r * 8 + k] -= f * m[c * 8 + k];
        inv[r * 8 + k] -= f * inv[c * 8 + k];
      }
    }
  }
}

// ---- XA tables (xa_kernels.hip, tools/xa_proto.py): all-pole cascades in DF-I state
// (y_k[t-1], y_k[t-2]) per section, real modal bases, the 25-tap FIR and frame-end forms ----
struct ApD {
  double a1[4], a2[4];
};
void ap_step_d(const ApD &c, const double in[8], double u, double out[8], double *y) {
  double s[8];
  for (int i = 0; i < 8; ++i) s[i] = in[i];
  double x = u;
  for (int k = 0; k < 4; ++k) {
    const double yy = x - c.a1[k] * s[2 * k] - c.a2[k] * s[2 * k + 1];
    s[2 * k + 1] = s[2 * k];
    s[2 * k] = yy;
    x = yy;
  }
  for (int i = 0; i < 8; ++i) out[i] = s[i];
  *y = x;
}

// Real modal basis of a cascade state matrix A (block lower triangular: section k's state is
// driven by the outputs of sections < k).  Mode j = the pole pair of section j, lambda_j =
// sigma + i omega = (-a1 + i sqrt(4 a2 - a1^2)) / 2; its eigenvector v is zero on sections
// < j, the null vector of (A_jj - lambda) on section j and found by forward substitution
// below.  Columns (Re v, Im v) of T give T^-1 A T = diag([[sigma, omega], [-omega, sigma]]),
// so a power of A is a per-mode complex power.
void modal_basis(const Mat8 &A, const cd lam[4], Mat8 &T) {
  T.assign(64, 0.0);
  for (int j = 0; j < 4; ++j) {
    cd v[8] = {};
    const double p = A[(2 * j) * 8 + 2 * j], q = A[(2 * j) * 8 + 2 * j + 1];
    v[2 * j] = q;
    v[2 * j + 1] = lam[j] - p;
    for (int k = j + 1; k < 4; ++k) {
      cd r0 = 0, r1 = 0;
      for (int l = 2 * j; l < 2 * k; ++l) {
        r0 -= A[(2 * k) * 8 + l] * v[l];
        r1 -= A[(2 * k + 1) * 8 + l] * v[l];
      }
      const cd m00 = A[(2 * k) * 8 + 2 * k] - lam[j], m01 = A[(2 * k) * 8 + 2 * k + 1];
      const cd m10 = A[(2 * k + 1) * 8 + 2 * k], m11 = A[(2 * k + 1) * 8 + 2 * k + 1] - lam[j];
      const cd det = m00 * m11 - m01 * m10;
      v[2 * k] = (r0 * m11 - m01 * r1) / det;
      v[2 * k + 1] = (m00 * r1 - m10 * r0) / det;
    }
    double nrm = 0;
    int big = 0;
    for (int i = 0; i < 8; ++i) {
      nrm += std::norm(v[i]);
      if (std::abs(v[i]) > std::abs(v[big])) big = i;
    }
    const cd rot = std::conj(v[big]) / std::abs(v[big]) / std::sqrt(nrm);
    for (int i = 0; i < 8; ++i) {
      const cd w = v[i] * rot;
      T[i * 8 + 2 * j] = w.real();
      T[i * 8 + 2 * j + 1] = w.imag();
    }
  }
}

// One pass: fills P, the output table cm (steps rows) and, when lag != nullptr, the
// far-field rows C A^d T for d < n_lag.
bool xa_pass_tables(const ApD &c, int steps, bool up, XaPass &P, float (*lag)[8], int n_lag, int B,
                    double (*lag_d)[8] = nullptr) {
  Mat8 A(64);
  double C[8];
  for (int q = 0; q < 8; ++q) {
    double e[8] = {0}, s2[8], y;
    e[q] = 1.0;
    ap_step_d(c, e, 0.0, s2, &y);
    for (int r = 0; r < 8; ++r) A[r * 8 + q] = s2[r];
    C[q] = y;
  }
  cd lam[4];
  for (int j = 0; j < 4; ++j) lam[j] = cd(-0.5 * c.a1[j], std::sqrt(c.a2[j] - 0.25 * c.a1[j] * c.a1[j]));
  Mat8 T, Ti;
  modal_basis(A, lam, T);
  mat_inverse8(T, Ti);
  double st[8], x = 1.0;
  for (int k = 0; k < 4; ++k) {
    P.a1[k] = (float)c.a1[k];
    P.a2[k] = (float)c.a2[k];
    x /= 1.0 + c.a1[k] + c.a2[k];
    st[2 * k] = st[2 * k + 1] = x;
  }
  for (int r = 0; r < 8; ++r) {
    double acc = 0;
    for (int k = 0; k < 8; ++k) acc += Ti[r * 8 + k] * st[k];
    P.ss[r] = (float)acc;
    for (int k = 0; k < 8; ++k) {
      P.ti[r][k] = (float)Ti[r * 8 + k];
      P.t[r][k] = (float)T[r * 8 + k];
    }
  }
  for (int j = 0; j < 4; ++j) {
    // the kernel's truncated scan must reach fp32-negligible powers for every mode
    if (std::pow(std::abs(lam[j]), (double)(steps << xa_levels(B, j))) > 1e-9) return false;
    const cd w = std::pow(lam[j], steps);
    P.pS[j][0] = (float)w.real();
    P.pS[j][1] = (float)w.imag();
    for (int d = 0; d < 4; ++d) {
      const cd u = std::pow(lam[j], steps << d);
      P.scan[d][j][0] = (float)u.real();
      P.scan[d][j][1] = (float)u.imag();
    }
  }
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 4; ++j) P.xr[i][j] = 0.f;
  for (int j = 0; j < kXaRowModes; ++j) {
    if (xa_levels(B, j) > 4) return false;  // row shifts reach at most 8 lanes
    for (int i = 0; i < 16; ++i) {
      const cd u = std::pow(lam[j], steps * (up ? i + 1 : 16 - i));
      P.xr[i][2 * j] = (float)u.real();
      P.xr[i][2 * j + 1] = (float)u.imag();
    }
  }
  Mat8 AtT = T;  // A^t T
  for (int t = 0; lag && t < n_lag; ++t) {
    for (int q = 0; q < 8; ++q) {
      double acc = 0;
      for (int r = 0; r < 8; ++r) acc += C[r] * AtT[r * 8 + q];
      lag[t][q] = (float)acc;
      if (lag_d) lag_d[t][q] = acc;
    }
    AtT = matmul8(A, AtT);
  }
  return true;
}
}  // namespace

bool xa_build_tables(XaTab &X, int B) {
  // sections slowest pole first (the lower-error fp32 order; any order is exact)
  ApD fw, bw;
  for (int k = 0; k < 4; ++k) {
    const double a1 = kDecimSos[3 - k][4], a2 = kDecimSos[3 - k][5];
    fw.a1[k] = a1;
    fw.a2[k] = a2;
    bw.a1[k] = 2.0 * a2 - a1 * a1;  // D(z) D(-z) = D2(z^2)
    bw.a2[k] = a2 * a2;
  }
  if (B != kXaB) return false;
  static double fcat[kXaB][8];
  if (!xa_pass_tables(fw, B, true, X.f, X.fcat, B, B, fcat) ||
      !xa_pass_tables(bw, B / 2, false, X.b, X.lag, kXaLag, B))
    return false;
  // N = b0 (1 + z^-1)^8 (sections 1..3 are exactly [1, 2, 1], section 0 is b0 [1, 2, 1])
  double n9[9], dneg[9] = {1.0}, mp[17] = {0}, m25[25] = {0};
  const double b0 = kDecimSos[0][0];
  for (int i = 0; i < 9; ++i) {
    double bin = 1.0;
    for (int r = 0; r < i; ++r) bin = bin * (8 - r) / (r + 1);
    n9[i] = b0 * bin;
  }
  int len = 1;
  for (int k = 0; k < 4; ++k) {  // D(-z) = prod (1 - a1 z^-1 + a2 z^-2)
    const double c1 = -kDecimSos[k][4], c2 = kDecimSos[k][5];
    double nx[9] = {0};
    for (int i = 0; i < len; ++i) {
      nx[i] += dneg[i];
      nx[i + 1] += c1 * dneg[i];
      nx[i + 2] += c2 * dneg[i];
    }
    len += 2;
    for (int i = 0; i < len; ++i) dneg[i] = nx[i];
  }
  for (int i = 0; i < 9; ++i)
    for (int k = 0; k < 9; ++k) mp[i + k] += n9[i] * dneg[k];   // taps on f[j + t]
  for (int t = 0; t < 17; ++t)
    for (int i = 0; i < 9; ++i) m25[t + i] += mp[t] * n9[8 - i];  // taps on v[j - 8 + u]
  double mps = 0, vss = 1.0;
  for (int t = 0; t < 17; ++t) {
    X.mp17[t] = (float)mp[t];
    mps += mp[t];
  }
  for (int u = 0; u < 25; ++u) X.m25[u] = (float)m25[u];
  // the zero-input responses through the FIR (xa_kernels.hip): output k of a lane takes
  // taps m25[24 + t - 1 - 2k] on its own v[t]; its share of the next lane's output k takes
  // m25[t - (B - 24) - 1 - 2k] on its v[t], t >= B - 23
  for (int k = 0; k < B / 2; ++k)
    for (int r = 0; r < 8; ++r) {
      double g = 0;
      for (int t = 0; t < B; ++t) {
        const int tap = 24 + t - 1 - 2 * k;
        if (tap >= 0 && tap < 25) g += m25[tap] * fcat[t][r];
      }
      X.gown[k][r] = (float)g;
    }
  for (int k = 0; k < 12; ++k)
    for (int r = 0; r < 8; ++r) {
      double g = 0;
      for (int t = B - 23; t < B; ++t) {
        const int tap = t - (B - 24) - 1 - 2 * k;
        if (tap >= 0 && tap < 25) g += m25[tap] * fcat[t][r];
      }
      X.gnb[k][r] = (float)g;
    }
  for (int i = 0; i < 9; ++i) X.n9[i] = (float)n9[i];
  for (int k = 0; k < 4; ++k) vss /= 1.0 + fw.a1[k] + fw.a2[k];
  X.mp_sum = (float)mps;
  X.vss = (float)vss;
  X.pad_[0] = X.pad_[1] = 0.f;
  return true;
}

}  // namespace zfft
