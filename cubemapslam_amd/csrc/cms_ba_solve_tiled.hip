// cms_ba_solve_tiled.hip -- dense LDL^T solve of the reduced camera system over many workgroups (global bundle adjustment,
// Optimizer.cpp:453-621: the map's free key frames give n = 6 np in the thousands, where k_ba_solve's one workgroup takes seconds).
//
// Right-looking, unpivoted, tile size BA_TL_NB, in place on the lower triangle of the row-major n x n matrix.  Per block column j:
//   k_ba_tl_factor   one workgroup      A_jj = L_jj D_j L_jj^T in LDS; d -> Dg, L_jj -> A (strictly lower part)
//   k_ba_tl_panel    one per tile row   W_ij = A_ij L_jj^-T (= L_ij D_j), L_ij = W_ij D_j^-1 -> A; both also k-major into the workspace
//   k_ba_tl_update   one wavefront per tile (i, k), i >= k > j:   A_ik -= W_ij L_kj^T on v_mfma_f64_16x16x4_f64
// then per block column, ascending / descending:
//   k_ba_tl_forward  y_j = L_jj^-1 b_j in every workgroup (same bits), workgroup w takes its rows of b_i -= L_ij y_j, i > j
//   k_ba_tl_backward x_j = L_jj^-T z_j in every workgroup, workgroup w takes its columns of z_k -= L_jk^T x_j, k < j
// Launch boundaries are the only grid-wide synchronisation.  Every entry of A, b receives its updates in ascending j (backward: descending),
// each update is one fixed-order sum, so the result is the same bits from run to run.  A zero or non-finite pivot clears the status word;
// every later launch reads it first and returns, k_ba_tl_finish then writes x = 0 (k_ba_solve's contract).  Ragged last tiles (n % NB != 0)
// are predicated; the workspace is padded to whole tiles and the padding rows hold zeros.
#define BA_TL_NB 48
#define BA_TL_LD (BA_TL_NB + 1)      // LDS row stride: one thread per row walks its row without bank conflicts
#define BA_TL_MAX_N 16384            // (n * n must stay an int for k_ba_schur_init's indexing; 12 288 is the documented size)

typedef double ba_tl_v4d __attribute__((ext_vector_type(4)));

struct BaTl {
  int n, nt, npad;      // order, tiles per side, nt * NB
  double* A;            // n x n row-major, lower triangle
  double* x;            // right-hand side in, solution out (in place)
  double* Dg;           // npad
  double* z;            // npad: D^-1 L^-1 b, the backward pass's right-hand side (never the vector a launch's other workgroups still read)
  double* Wt;           // NB x npad: (L_ij D_j), k-major, of the current block column
  double* Lt;           // NB x npad: L_ij, k-major
  int* status;
};

// status = 1, x = b
extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_init(BaTl t, const double* __restrict__ b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *t.status = 1;
  if (i < t.n) t.x[i] = b[i];
}

extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_factor(BaTl t, int j) {
  __shared__ double T[BA_TL_NB * BA_TL_LD];
  __shared__ double ucol[BA_TL_NB], lcol[BA_TL_NB];
  __shared__ int bad;
  if (*t.status == 0) return;
  const int tid = threadIdx.x, n = t.n, r0 = j * BA_TL_NB, nb = min(BA_TL_NB, n - r0);
  if (tid == 0) bad = 0;
  for (int e = tid; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    T[r * BA_TL_LD + c] = c <= r ? t.A[(size_t)(r0 + r) * n + r0 + c] : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < nb; ++c) {
    const double d = T[c * BA_TL_LD + c];
    if (tid == 0 && (!isfinite(d) || d == 0.0)) bad = 1;
    for (int r = c + 1 + tid; r < nb; r += 256) {
      const double a = T[r * BA_TL_LD + c];
      ucol[r] = a;              // a_rc (unscaled)
      lcol[r] = a / d;          // l_rc
    }
    __syncthreads();
    if (bad) break;
    const int rem = nb - c - 1;
    for (int e = tid; e < rem * rem; e += 256) {
      const int r = c + 1 + e / rem, s = c + 1 + e % rem;
      if (s <= r) T[r * BA_TL_LD + s] -= lcol[r] * ucol[s];
    }
    for (int r = c + 1 + tid; r < nb; r += 256) T[r * BA_TL_LD + c] = lcol[r];
    __syncthreads();
  }
  if (bad) { if (tid == 0) *t.status = 0; return; }
  for (int e = tid; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    if (c < r) t.A[(size_t)(r0 + r) * n + r0 + c] = T[r * BA_TL_LD + c];
    else if (c == r) t.Dg[r0 + r] = T[r * BA_TL_LD + c];
  }
}

// tile row i = j + 1 + blockIdx.x (block column j is a full tile whenever it has a panel below it)
extern "C" __global__ void __launch_bounds__(64)
k_ba_tl_panel(BaTl t, int j) {
  __shared__ double Lj[BA_TL_NB * BA_TL_LD], T[BA_TL_NB * BA_TL_LD], Wd[BA_TL_NB * BA_TL_LD], dg[BA_TL_NB];
  if (*t.status == 0) return;
  const int tid = threadIdx.x, n = t.n, c0 = j * BA_TL_NB, i = j + 1 + blockIdx.x, r0 = i * BA_TL_NB;
  for (int e = tid; e < BA_TL_NB * BA_TL_NB; e += 64) {
    const int r = e / BA_TL_NB, c = e % BA_TL_NB;
    Lj[r * BA_TL_LD + c] = c < r ? t.A[(size_t)(c0 + r) * n + c0 + c] : 0.0;
    T[r * BA_TL_LD + c] = r0 + r < n ? t.A[(size_t)(r0 + r) * n + c0 + c] : 0.0;
  }
  if (tid < BA_TL_NB) dg[tid] = t.Dg[c0 + tid];
  __syncthreads();
  if (tid < BA_TL_NB) {
    double* row = T + tid * BA_TL_LD;
    double* wrow = Wd + tid * BA_TL_LD;
    for (int c = 0; c < BA_TL_NB; ++c) {
      double w = row[c];
      const double* lc = Lj + c * BA_TL_LD;
      for (int k = 0; k < c; ++k) w -= wrow[k] * lc[k];       // w_rc = a_rc - sum_k<c w_rk l_ck
      wrow[c] = w;
      row[c] = w / dg[c];
    }
  }
  __syncthreads();
  for (int e = tid; e < BA_TL_NB * BA_TL_NB; e += 64) {
    const int r = e / BA_TL_NB, c = e % BA_TL_NB;
    if (r0 + r < n) t.A[(size_t)(r0 + r) * n + c0 + c] = T[r * BA_TL_LD + c];
  }
  for (int e = tid; e < BA_TL_NB * BA_TL_NB; e += 64) {      // k-major copies: consecutive lanes, consecutive rows (rows >= n: zeros)
    const int c = e / BA_TL_NB, r = e % BA_TL_NB;
    t.Wt[(size_t)c * t.npad + r0 + r] = Wd[r * BA_TL_LD + c];
    t.Lt[(size_t)c * t.npad + r0 + r] = T[r * BA_TL_LD + c];
  }
}

// Trailing update of step j: tile number w (one wavefront each) of the lower triangle of the (nt - j - 1)^2 trailing tiles, 3 x 3 MFMA
// tiles of 16 x 16, 12 steps of 4 along the panel's 48 columns.  Operands (cdna4: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15])
// come straight from the k-major panel copies; C/D is col = lane & 15, row = (lane >> 4) + 4 reg.
extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_update(BaTl t, int j, int ntiles) {
  if (*t.status == 0) return;
  const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= ntiles) return;
  int ti = (int)((sqrt(8.0 * (double)w + 1.0) - 1.0) * 0.5);
  while ((ti + 1) * (ti + 2) / 2 <= w) ++ti;
  while (ti * (ti + 1) / 2 > w) --ti;
  const int tk = w - ti * (ti + 1) / 2;
  const int n = t.n, r0 = (j + 1 + ti) * BA_TL_NB, c0 = (j + 1 + tk) * BA_TL_NB;
  const int lr = lane >> 4, lc = lane & 15;
  ba_tl_v4d acc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = r0 + 16 * a + lr + 4 * g, col = c0 + 16 * b + lc;
        acc[a][b][g] = (row < n && col <= row) ? t.A[(size_t)row * n + col] : 0.0;
      }
  const double* wp = t.Wt + r0 + lc;
  const double* lp = t.Lt + c0 + lc;
#pragma unroll 2
  for (int kk = 0; kk < BA_TL_NB / 4; ++kk) {
    const size_t o = (size_t)(4 * kk + lr) * t.npad;
    double wa[3], lb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { wa[a] = -wp[o + 16 * a]; lb[a] = lp[o + 16 * a]; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[a], lb[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = r0 + 16 * a + lr + 4 * g, col = c0 + 16 * b + lc;
        if (row < n && col <= row) t.A[(size_t)row * n + col] = acc[a][b][g];
      }
}

// unit lower triangle of tile (j, j) -> LDS (zero above the diagonal and beyond nb)
__device__ __forceinline__ void ba_tl_load_diag(const BaTl& t, int j, int nb, double* Lj) {
  const int r0 = j * BA_TL_NB;
  for (int e = threadIdx.x; e < BA_TL_NB * BA_TL_NB; e += blockDim.x) {
    const int r = e / BA_TL_NB, c = e % BA_TL_NB;
    Lj[r * BA_TL_LD + c] = (c < r && r < nb) ? t.A[(size_t)(r0 + r) * t.n + r0 + c] : 0.0;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_forward(BaTl t, int j) {
  __shared__ double Lj[BA_TL_NB * BA_TL_LD], y[BA_TL_NB];
  if (*t.status == 0) return;
  const int tid = threadIdx.x, n = t.n, r0 = j * BA_TL_NB, nb = min(BA_TL_NB, n - r0);
  ba_tl_load_diag(t, j, nb, Lj);
  if (tid < BA_TL_NB) y[tid] = tid < nb ? t.x[r0 + tid] : 0.0;
  __syncthreads();
  if (tid < 64) {      // one wavefront, column oriented: its LDS operations are in order
    for (int c = 0; c < nb - 1; ++c) {
      const double yc = y[c];
      if (tid > c && tid < nb) y[tid] -= Lj[tid * BA_TL_LD + c] * yc;
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  const int row = r0 + BA_TL_NB + blockIdx.x * 256 + tid;
  if (row < n) {
    const double* a = t.A + (size_t)row * n + r0;
    double s = t.x[row];
    for (int c = 0; c < BA_TL_NB; ++c) s -= a[c] * y[c];
    t.x[row] = s;
  }
  if (blockIdx.x == 0 && tid < nb) t.z[r0 + tid] = y[tid] / t.Dg[r0 + tid];      // z = D^-1 y (x[r0..] itself is still being read by the other workgroups)
}

extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_backward(BaTl t, int j) {
  __shared__ double Lj[BA_TL_NB * BA_TL_LD], xs[BA_TL_NB];
  if (*t.status == 0) return;
  const int tid = threadIdx.x, n = t.n, r0 = j * BA_TL_NB, nb = min(BA_TL_NB, n - r0);
  ba_tl_load_diag(t, j, nb, Lj);
  if (tid < BA_TL_NB) xs[tid] = tid < nb ? t.z[r0 + tid] : 0.0;
  __syncthreads();
  if (tid < 64) {
    for (int c = nb - 1; c > 0; --c) {      // L_jj^T x = z, column oriented
      const double xc = xs[c];
      if (tid < c) xs[tid] -= Lj[c * BA_TL_LD + tid] * xc;
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  const int col = blockIdx.x * 256 + tid;
  if (col < r0) {
    double s = t.z[col];
    for (int r = 0; r < nb; ++r) s -= t.A[(size_t)(r0 + r) * n + col] * xs[r];
    t.z[col] = s;
  }
  if (blockIdx.x == 0 && tid < nb) t.x[r0 + tid] = xs[tid];
}

extern "C" __global__ void __launch_bounds__(256)
k_ba_tl_finish(BaTl t) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (*t.status == 0 && i < t.n) t.x[i] = 0.0;
}

// workspace doubles for order n: Dg + z + Wt + Lt (ba_tl_bind cuts them)
static size_t ba_tl_ws_doubles(int n) {
  const size_t npad = (size_t)((n + BA_TL_NB - 1) / BA_TL_NB) * BA_TL_NB;
  return npad * (2 + 2 * (size_t)BA_TL_NB);
}
static BaTl ba_tl_bind(int n, double* A, double* x, double* ws, int* status) {
  BaTl t;
  t.n = n; t.nt = (n + BA_TL_NB - 1) / BA_TL_NB; t.npad = t.nt * BA_TL_NB;
  t.A = A; t.x = x; t.Dg = ws; t.z = ws + t.npad; t.Wt = ws + 2 * (size_t)t.npad; t.Lt = t.Wt + (size_t)BA_TL_NB * t.npad; t.status = status;
  return t;
}
// the whole solve, enqueued on `s` (nothing is waited for).  A is overwritten, x receives the solution (or zeros), *status 1 / 0.
static void ba_tl_enqueue(const BaTl& t, const double* b, hipStream_t s) {
  const int n = t.n, nt = t.nt;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_ba_tl_init, dim3((n + 255) / 256), dim3(256), 0, s, t, b);
  for (int j = 0; j < nt; ++j) {
    hipLaunchKernelGGL(k_ba_tl_factor, dim3(1), dim3(256), 0, s, t, j);
    const int m = nt - j - 1;
    if (m <= 0) continue;
    hipLaunchKernelGGL(k_ba_tl_panel, dim3(m), dim3(64), 0, s, t, j);
    const int ntiles = m * (m + 1) / 2;
    hipLaunchKernelGGL(k_ba_tl_update, dim3((ntiles + 3) / 4), dim3(256), 0, s, t, j, ntiles);
  }
  for (int j = 0; j < nt; ++j) {
    const int below = n - (j + 1) * BA_TL_NB;
    hipLaunchKernelGGL(k_ba_tl_forward, dim3(std::max(1, (below + 255) / 256)), dim3(256), 0, s, t, j);
  }
  for (int j = nt - 1; j >= 0; --j)
    hipLaunchKernelGGL(k_ba_tl_backward, dim3(std::max(1, (j * BA_TL_NB + 255) / 256)), dim3(256), 0, s, t, j);
  hipLaunchKernelGGL(k_ba_tl_finish, dim3((n + 255) / 256), dim3(256), 0, s, t);
}
