// The alignment of the flight recorder's trajectory error (vi_ekf_amd/csrc/viekf_rec_align.hpp) is plain arithmetic for host and
// device alike: this program includes only that header and holds it, without a device, against rotations it knows.
//   1. sweeps: over 20000 matrices A (random, rank-deficient, scaled between 1e-12 and 1e+12) the off-diagonal norm of Horn's
//      matrix relative to its Frobenius norm after 1 .. kRecJacobiSweeps sweeps; the header's comment quotes what this prints.
//   2. se3: A built from points moved by a known rotation gives that rotation back (unit, w >= 0), and the result maximises
//      tr(R A^T) against perturbed rotations when the points carry noise.
//   3. yaw: the closed form against a known yaw, and theta = 0 when both arguments vanish.
#include <algorithm>
#include <cstdio>
#include <random>

#include "../../vi_ekf_amd/csrc/viekf_rec_align.hpp"

using namespace viekf;

static void rot_of(const double* q, double (&R)[3][3]) {   // active: R v = q v q*
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - w * z);     R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z);     R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y);     R[2][1] = 2 * (y * z + w * x);     R[2][2] = 1 - 2 * (x * x + y * y);
}

static double trace_RAt(const double* q, const double* A) {
  double R[3][3], s = 0;
  rot_of(q, R);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) s += R[i][j] * A[3 * i + j];
  return s;
}

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> ud(-12.0, 12.0);
  int bad = 0;

  // 1. sweeps
  double worst[kRecJacobiSweeps + 1] = {0};
  for (int trial = 0; trial < 20000; trial++) {
    double A[9];
    for (double& a : A) a = nd(rng);
    if (trial % 4 == 1) for (int j = 0; j < 3; j++) A[6 + j] = 0.0;                       // planar
    if (trial % 4 == 2) for (int i = 1; i < 3; i++) for (int j = 0; j < 3; j++) A[3 * i + j] = A[j] * (i + 0.5);   // rank one
    const double sc = trial % 4 == 3 ? std::pow(10.0, ud(rng)) : 1.0;
    for (double& a : A) a *= sc;
    for (int sweeps = 1; sweeps <= kRecJacobiSweeps; sweeps++) {
      double N[4][4], V[4][4], fro = 0.0;
      rec_horn_matrix(A, N);
      for (auto& row : N) for (double v : row) fro += v * v;
      const double off = rec_jacobi4(N, V, sweeps);
      worst[sweeps] = std::max(worst[sweeps], fro > 0.0 ? off / std::sqrt(fro) : 0.0);
    }
  }
  for (int s = 1; s <= kRecJacobiSweeps; s++) std::printf("sweeps %d worst relative off-diagonal norm %.3e\n", s, worst[s]);
  bad += !(worst[kRecJacobiSweeps - 2] <= 1e-15);   // two sweeps in hand

  // 2. se3
  double worst_rot = 0.0;
  for (int trial = 0; trial < 2000; trial++) {
    double q[4], nq = 0.0;
    for (double& v : q) { v = nd(rng); nq += v * v; }
    for (double& v : q) v /= std::sqrt(nq);
    if (q[0] < 0) for (double& v : q) v = -v;
    double R[3][3];
    rot_of(q, R);
    const int n = 4 + trial % 60;
    const double noise = trial % 2 ? 0.02 : 0.0;
    double A[9] = {0};
    for (int k = 0; k < n; k++) {
      double e[3], t[3];
      for (double& v : e) v = nd(rng);
      for (int i = 0; i < 3; i++) t[i] = R[i][0] * e[0] + R[i][1] * e[1] + R[i][2] * e[2] + noise * nd(rng);
      for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A[3 * i + j] += t[i] * e[j];   // (the centring is the kernel's, not tested here)
    }
    double g[4];
    rec_align_se3(A, g);
    const double ng = g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
    bad += !(std::fabs(ng - 1.0) <= 1e-14) || !(g[0] >= 0.0);
    if (noise == 0.0) {
      double d = 0.0;
      for (int i = 0; i < 4; i++) d = std::max(d, std::fabs(g[i] - q[i]));
      worst_rot = std::max(worst_rot, d);
    } else {   // a maximiser: no rotation near it does better
      const double best = trace_RAt(g, A);
      for (int p = 0; p < 8; p++) {
        double h[4], nh = 0.0;
        for (int i = 0; i < 4; i++) { h[i] = g[i] + 1e-3 * nd(rng); nh += h[i] * h[i]; }
        for (double& v : h) v /= std::sqrt(nh);
        bad += !(trace_RAt(h, A) <= best + 1e-12 * std::fabs(best));
      }
    }
  }
  std::printf("se3: a known rotation comes back to %.3e\n", worst_rot);
  bad += !(worst_rot <= 1e-13);

  // 3. yaw
  for (int trial = 0; trial < 200; trial++) {
    const double th = 3.0 * nd(rng) / 3.0;
    double A[9] = {0};
    for (int k = 0; k < 10; k++) {
      const double e[3] = {nd(rng), nd(rng), nd(rng)};
      const double t[3] = {std::cos(th) * e[0] - std::sin(th) * e[1], std::sin(th) * e[0] + std::cos(th) * e[1], e[2]};
      for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A[3 * i + j] += t[i] * e[j];
    }
    double g[4];
    rec_align_yaw(A, g);
    const double back = 2.0 * std::atan2(g[3], g[0]);
    bad += !(std::fabs(std::remainder(back - th, 6.283185307179586)) <= 1e-14) || g[1] != 0.0 || g[2] != 0.0;
  }
  const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 5.0};
  double g[4];
  rec_align_yaw(Z, g);
  bad += !(g[0] == 1.0 && g[3] == 0.0);
  const double O[9] = {0};
  rec_align_se3(O, g);
  bad += !(g[0] == 1.0 && g[1] == 0.0 && g[2] == 0.0 && g[3] == 0.0);   // one frame: A = 0 gives the identity

  if (bad) { std::fprintf(stderr, "rec align model: %d checks failed\n", bad); return 1; }
  std::printf("rec align model: ok\n");
  return 0;
}
