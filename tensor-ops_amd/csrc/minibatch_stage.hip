// The staging in front of the steps of to_fflayer_stack_minibatch_sgd (stack_ff.cpp): the rows of a chunk of consecutive
// minibatches, gathered through the device's copy of the caller's index table into per-step slabs of one pool buffer.
//   dst_x[(r / M) * x_slab + (r % M) * x_row ..] = X[idx[r]][..]     r < n_rows      (and the same for Y when there is one)
// ONE launch a chunk gathers both tensors.  A wave takes whole rows (grid-stride over the rows), its lanes the pieces of
// the row; a row's index is read once a wave and is wave-uniform, so is the slab it lands in.  Each tensor moves in the
// widest piece its rows allow -- 16 bytes when the row bytes, the slab stride and both bases are multiples of 16, else one
// element -- chosen per tensor: X rows of 784 floats go 16 bytes a lane while Y rows of 10 floats go by element, in the same
// launch.  Plain vector loads and stores; nothing persistent, no workgroup talks to another.  The indices were checked on
// the host (stack_ff.cpp), and r < n_rows bounds every store inside the chunk's slabs.
#include <cstdint>

#include "common.hpp"

namespace to {

namespace {

struct alignas(16) Piece16 { unsigned v[4]; };
template <int W> struct PieceOf;
template <> struct PieceOf<4> { using type = unsigned; };
template <> struct PieceOf<8> { using type = unsigned long long; };
template <> struct PieceOf<16> { using type = Piece16; };

struct StageSide {
  const char* src;  // the resident tensor, rows `row` bytes apart (null: nothing to gather)
  char* dst;        // the first step's slab
  long row;         // bytes a row
  long slab;        // bytes between the slabs of consecutive steps
};

template <int W>
__device__ __forceinline__ void stage_row(const StageSide& t, long src_row, long step, long in_step, int lane) {
  using P = typename PieceOf<W>::type;
  const P* s = reinterpret_cast<const P*>(t.src + src_row * t.row);
  P* d = reinterpret_cast<P*>(t.dst + step * t.slab + in_step * t.row);
  const long n = t.row / W;
  for (long j = lane; j < n; j += 64) d[j] = s[j];
}

template <int WX, int WY>
__global__ __launch_bounds__(256) void minibatch_stage_kernel(StageSide x, StageSide y, const long long* __restrict__ idx,
                                                              long n_rows, long M) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (long)gridDim.x * 4;
  for (long r = wave; r < n_rows; r += waves) {
    const long src_row = idx[r], step = r / M, in_step = r - step * M;
    stage_row<WX>(x, src_row, step, in_step, lane);
    if constexpr (WY != 0) stage_row<WY>(y, src_row, step, in_step, lane);
  }
}

int piece_width(const StageSide& t, int es) {
  const bool wide = t.row % 16 == 0 && t.slab % 16 == 0 && (reinterpret_cast<uintptr_t>(t.src) & 15u) == 0 &&
                    (reinterpret_cast<uintptr_t>(t.dst) & 15u) == 0;
  return wide ? 16 : es;
}

}  // namespace

void launch_minibatch_stage(const long long* idx, int64_t n_rows, int64_t M, const void* X, void* x_dst, int64_t x_row_bytes,
                            int64_t x_slab_bytes, const void* Y, void* y_dst, int64_t y_row_bytes, int64_t y_slab_bytes,
                            int es, hipStream_t s) {
  if (n_rows == 0) return;
  TO_CHECK((es == 4 || es == 8) && M >= 1 && x_row_bytes % es == 0 && (!Y || y_row_bytes % es == 0), TO_ERR_STATE,
           "internal: minibatch stage arguments");
  const StageSide x{static_cast<const char*>(X), static_cast<char*>(x_dst), (long)x_row_bytes, (long)x_slab_bytes};
  const StageSide y{static_cast<const char*>(Y), static_cast<char*>(y_dst), (long)y_row_bytes, (long)y_slab_bytes};
  const int wx = piece_width(x, es), wy = Y ? piece_width(y, es) : 0;
  long blocks = (long)((n_rows + 3) / 4);   // four waves a workgroup, a row a wave; the rest by grid stride
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks), block(256);
#define TOPS_STAGE(WX, WY) launch_k((minibatch_stage_kernel<WX, WY>), grid, block, 0, s, x, y, idx, (long)n_rows, (long)M)
#define TOPS_STAGE_Y(WX)                                                                   \
  do {                                                                                     \
    if (wy == 16) TOPS_STAGE(WX, 16); else if (wy == 8) TOPS_STAGE(WX, 8);                 \
    else if (wy == 4) TOPS_STAGE(WX, 4); else TOPS_STAGE(WX, 0);                           \
  } while (0)
  if (wx == 16) TOPS_STAGE_Y(16);
  else if (wx == 8) TOPS_STAGE_Y(8);
  else TOPS_STAGE_Y(4);
#undef TOPS_STAGE_Y
#undef TOPS_STAGE
  TO_HIP(hipGetLastError());
  count_launch();
}

}  // namespace to
