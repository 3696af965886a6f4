// The fp64 pair-tile walker shared by manifold.hip (squared distances), kid.hip (polynomial kernel values) and mmd.hip
// (kernel values of centred rows, times blocks of indicators): a workgroup of 256 threads owns 64 row positions and walks a
// range of 64-wide column tiles of a matrix of dot products g_ij = b_i . a_j of rows (fp32, or double where a caller keeps
// them so: the type that Rows::b returns), converted to double on load; every finished tile goes through LDS to the caller's
// epilogue and the matrix is never written to memory.  g_ij has one summation order: features in order, no split over F.
//   v_mfma_f64_16x16x4_f64 (f64_tile.hpp: f64_mfma_slab; lane layout there), 64 x 64 tile per workgroup, 32 x 32 per wave,
//   32 features per staged step.
//   Staging: a thread holds the features k0 + tid % 32 of the rows tid / 32 + 8 e, e < 8, of each operand.  The fp32 elements
//   of the next step (of the next tile after a tile's last step) are fetched into registers while the MFMAs of this one run.
//   LDS: the 64 x 68 result tile; the two staged operands (32 x 66 each) live in its first doubles, so a tile's values are
//   written only after a barrier behind its last MFMAs.  The +2 / +4 of the row strides spread the staging writes and the
//   epilogue's 16 rows x 4 quarters of a wave over the banks.
//   Epilogue: thread e = 4 row + quarter reads the columns quarter, quarter + 4, ... of its row, lds[row * PT_LDD + column];
//   the four quarters of a row are four neighbouring lanes.
// The callers differ in two policies, every member __forceinline__ (Rows is taken by value: the walker owns its copy):
//   Rows      columns(j0)                 before the first fetch of the column tile at j0
//             b(e, k0), a(e, j0, k0)      the thread's element e (fp32 or double) of the step at feature k0: feature k0 + tid % 32 of row
//                                         tid / 32 + 8 e of the row tile / of the column tile at j0; 0 outside the operand
//                                         (e is a constant after unrolling)
//   Epilogue  stage(t)                    before the values of column tile t are written (what its readers need beside it)
//             column(t, cj)               what the values of column cj of the tile share (read once per column; any type)
//             element(col, ci, g)         the value of the tile at row ci of that column from its dot product g
//             tile(lds, t)                after the barrier behind the writes: the thread takes its quarter of its row
#pragma once
#include "f64_tile.hpp"

#define PT_TILE 64                 // tile of a workgroup: row positions x column positions
#define PT_KT 32                   // feature depth of a staged step
#define PT_LDS (PT_TILE + 2)       // LDS row stride of a staged operand, in doubles
#define PT_LDD (PT_TILE + 4)       // LDS row stride of the result tile
#define PT_LOADS (PT_TILE * PT_KT / 256)      // elements of each operand a thread stages per step
#define PT_SLOTS 512               // workgroups wanted in flight: 256 CUs x 2 (34.8 KB of LDS each)
#define PT_MIN_TILES 4             // column tiles per chunk at least (a chunk ends in a merge of four partials per row)

static __host__ __device__ int pt_tiles(long n) { return (int)((n + PT_TILE - 1) / PT_TILE); }

// How many workgroups share a row's `col_tiles` column tiles -> column tiles per chunk and the chunks that hold at least one
// tile.  `chunks` 0, the default plan: as many chunks as fill `slots` workgroups, given the `groups_unsplit` of an unsplit
// launch, of at least `min_tiles` tiles each.
static void pair_plan(long groups_unsplit, int col_tiles, int chunks, int slots, int min_tiles, int* tiles_per_chunk,
                      int* n_chunks) {
  if (chunks <= 0) {
    chunks = (int)((slots + groups_unsplit - 1) / groups_unsplit);
    const int most = (col_tiles + min_tiles - 1) / min_tiles;
    if (chunks > most) chunks = most;
  }
  if (chunks > col_tiles) chunks = col_tiles;
  *tiles_per_chunk = (col_tiles + chunks - 1) / chunks;
  *n_chunks = (col_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// the column tiles [t0, t1) against the workgroup's row tile; all 256 threads call it (barriers inside)
template <class Rows, class Epilogue>
__device__ __forceinline__ void pair_tile_walk(Rows rows, Epilogue& epi, int F, int t0, int t1) {
  __shared__ double lds[PT_TILE * PT_LDD];      // the result tile; the staged operands live in its first 2 PT_KT PT_LDS doubles
  double(*Bs)[PT_LDS] = reinterpret_cast<double(*)[PT_LDS]>(lds);
  double(*As)[PT_LDS] = reinterpret_cast<double(*)[PT_LDS]>(lds + PT_KT * PT_LDS);
  static_assert(2 * PT_KT * PT_LDS <= PT_TILE * PT_LDD, "the staged operands fit inside the result tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  const int frow = tid / PT_KT, fk = tid % PT_KT;
  using elem_t = decltype(rows.b(0, 0));      // fp32 (manifold, kid) or double (mmd: rows centred in double)
  elem_t pb[PT_LOADS], pa[PT_LOADS];
  auto fetch = [&](long j0, int k0) {
#pragma unroll
    for (int e = 0; e < PT_LOADS; ++e) {
      pb[e] = rows.b(e, k0);
      pa[e] = rows.a(e, j0, k0);
    }
  };
  if (t0 < t1) {
    rows.columns((long)t0 * PT_TILE);
    fetch((long)t0 * PT_TILE, 0);
  }
  for (int t = t0; t < t1; ++t) {
    const long j0 = (long)t * PT_TILE;
    f64x4 acc[2][2] = {};
    for (int k0 = 0; k0 < F; k0 += PT_KT) {
      __syncthreads();      // (the previous tile's epilogue, or the previous step's MFMAs, have read the LDS)
#pragma unroll
      for (int e = 0; e < PT_LOADS; ++e) {
        const int r = frow + (256 / PT_KT) * e;
        Bs[fk][r] = (double)pb[e];
        As[fk][r] = (double)pa[e];
      }
      __syncthreads();
      if (k0 + PT_KT < F) {
        fetch(j0, k0 + PT_KT);
      } else if (t + 1 < t1) {
        rows.columns(j0 + PT_TILE);
        fetch(j0 + PT_TILE, 0);
      }
      f64_mfma_slab<PT_KT, PT_LDS, 2>(Bs, As, wm, wn, lr, lk, acc);
    }
    __syncthreads();        // (the last MFMAs have read the staged operands the tile overwrites)
    epi.stage(t);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cj = wn + 16 * ni + lr;
      const auto col = epi.column(t, cj);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = wm + 16 * mi + lk + 4 * r;
          lds[ci * PT_LDD + cj] = epi.element(col, ci, acc[mi][ni][r]);
        }
    }
    __syncthreads();
    epi.tile(lds, t);
  }
}
