// bx_embtile.h — the dets_embs @ trk_embs.T tile BoostTrack and DeepOCSort share, on the fp64
// matrix cores.  One workgroup of 4 waves per output tile of 32 detections x 64 tracks (wave
// (wr, wc): rows 16 wr, columns 32 wc + {0, 16}); K advances in chunks of 16 through LDS stored
// k-major, with EC_PF chunks' global loads in flight (a chunk's MFMAs take ~50 ns, a load round
// trip ~1 us: the loop is bound by how many round trips it waits for).  Entry (d, p) = ascending-k
// fma chain over F (oracle emb_dot); F is any positive width (the K tail is zero-filled, and
// x + 0 * 0 leaves a chain's value unchanged).
// Included inside the including translation unit's anonymous namespace.
constexpr int EC_BM = 32, EC_BN = 64, EC_KC = 16, EC_LDA = EC_BM + 16, EC_LDB = EC_BN + 16;
constexpr int EC_STAGE = EC_KC * (EC_LDA + EC_LDB);
#ifndef BX_EC_PF
#define BX_EC_PF 4
#endif
constexpr int EC_PF = BX_EC_PF;  // chunks in flight
typedef double d4 __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int ec_tiles_t(int T) { return (T + EC_BN - 1) / EC_BN; }
__host__ __device__ constexpr int ec_tiles(int D, int T) {
  return (D + EC_BM - 1) / EC_BM * ec_tiles_t(T);
}

// Staging roles of thread `tid` of the 256: A 32 rows x 16 k (8 threads x 2 per row), B 64 rows x
// 16 k (4 threads x 4).  ec_tile takes the thread's row pointers already advanced by its k offset.
__device__ __forceinline__ int ec_arow(int tid) { return tid >> 3; }
__device__ __forceinline__ int ec_ak(int tid) { return (tid & 7) * 2; }
__device__ __forceinline__ int ec_brow(int tid) { return tid >> 2; }
__device__ __forceinline__ int ec_bk(int tid) { return (tid & 3) * 4; }

// lds: 2 * EC_STAGE doubles.  ap / bp: row ec_arow of A / ec_brow of B of this tile, + ec_ak /
// ec_bk (read only where a_ok / b_ok).  acc[j][q] = entry (16 wr + lane / 16 + 4 q,
// 32 wc + 16 j + lane % 16) of the tile.
__device__ __forceinline__ void ec_tile(double* lds, int F, bool a_ok, const double* ap, bool b_ok,
                                        const double* bp, d4* acc) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int ar = ec_arow(tid), aq = ec_ak(tid), br = ec_brow(tid), bq = ec_bk(tid);
  const int nk = (F + EC_KC - 1) / EC_KC;
  double ra[EC_PF][2], rb[EC_PF][4];
  auto load = [&](int sl, int kc) {
    const int k0 = kc * EC_KC;
#pragma unroll
    for (int j = 0; j < 2; j++) ra[sl][j] = (a_ok && k0 + aq + j < F) ? ap[k0 + j] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) rb[sl][j] = (b_ok && k0 + bq + j < F) ? bp[k0 + j] : 0.0;
  };
  auto store = [&](int sl, double* buf) {
#pragma unroll
    for (int j = 0; j < 2; j++) buf[(aq + j) * EC_LDA + ar] = ra[sl][j];
#pragma unroll
    for (int j = 0; j < 4; j++) buf[EC_KC * EC_LDA + (bq + j) * EC_LDB + br] = rb[sl][j];
  };
  acc[0] = (d4){0.0, 0.0, 0.0, 0.0};
  acc[1] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < EC_PF; p++)
    if (p < nk) load(p, p);
  store(0, lds);
  __syncthreads();
  // chunk kc sits in LDS stage kc & 1 and register slot kc % EC_PF (free once stored); the loop
  // is unrolled by EC_PF so the slots are static
  for (int kb = 0; kb < nk; kb += EC_PF) {
#pragma unroll
    for (int u = 0; u < EC_PF; u++) {
      const int kc = kb + u;
      if (kc < nk) {
        if (kc + EC_PF < nk) load(u, kc + EC_PF);
        const double* cur = lds + (kc & 1) * EC_STAGE;
#pragma unroll
        for (int ks = 0; ks < EC_KC / 4; ks++) {
          const int kr = ks * 4 + (lane >> 4);
          const double a = cur[kr * EC_LDA + wr * 16 + (lane & 15)];
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const double bb = cur[EC_KC * EC_LDA + kr * EC_LDB + wc * 32 + j * 16 + (lane & 15)];
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[j], 0, 0, 0);
          }
        }
        if (kc + 1 < nk) store((u + 1) % EC_PF, lds + ((kc + 1) & 1) * EC_STAGE);
        __syncthreads();
      }
    }
  }
}

// The tile's entries inside [nd] x [nt] to out[row * ld + col].
__device__ __forceinline__ void ec_tile_store(const d4* acc, int d0, int t0, int nd, int nt,
                                              double* out, int ld) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wc = w >> 1;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int col = t0 + wc * 32 + j * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = d0 + wr * 16 + (lane >> 4) + 4 * q;
      if (row < nd && col < nt) out[(size_t)row * ld + col] = acc[j][q];
    }
  }
}
