// What ehyb_cg.hip shares with a solver that keeps its CG recurrences and brings a preconditioner of its own (ehyb_cheb.hip):
// the slot layout of a column and the launches of its vector kernels, K columns wide.  The kernels live in ehyb_cg.hip alone.
#pragma once
#include <hip/hip_runtime.h>

namespace ehyb {

// partial arrays, kMaxGrid doubles each
// (r.r sits between the two r.z slots, so that the pair an iteration writes -- its new r.z and r.r -- is one
// contiguous range for a multi-GPU caller's all-reduce: slot of r.z number c = A_RZ0 + 2 c)
enum { A_BB = 0, A_PQ = 1, A_RZ0 = 2, A_RR = 3, A_RZ1 = 4, A_COUNT = 5 };

// One launch each for columns c0 .. c0 + K - 1 (K = 1..4), every column with its A_COUNT slots behind s; active: the columns'
// flags (null: K = 1, the column is live).
//   init       r = b - q, p = z = dinv .* r (or r); partials of r.z (slot A_RZ0), r.r, b.b.  One column.
//   dot        partials of p . q
//   update     alpha = r.z[cur] / p.q;  x += alpha p;  r -= alpha q;  partials of r.z[cur ^ 1] (z = dinv .* r, or r) and of r.r
//   direction  beta = r.z[cur ^ 1] / r.z[cur];  p = z + beta p, z = dinv .* Zv (or Zv)
void cg_launch_init(int grid, hipStream_t st, int n, const double* b, const double* q, const double* dinv, double* r, double* p, double* s);
void cg_launch_dot(int K, int grid, hipStream_t st, int n, const double* P, const double* Q, double* s, const int* active, int c0);
void cg_launch_update(int K, int grid, hipStream_t st, int n, const double* P, const double* Q, const double* dinv, double* X, long long ldx,
                      double* R, double* s, const int* active, int c0, int cur);
void cg_launch_direction(int K, int grid, hipStream_t st, int n, const double* Zv, const double* dinv, double* P, const double* s,
                         const int* active, int c0, int cur);

}  // namespace ehyb
