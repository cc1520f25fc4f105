// What read bandwidth does the access pattern of riccati_forward_kernel admit on this box?  4096 wavefronts (16 per CU, the
// forward kernel's launch), each reading 1.2 MB (1216 KB):
//   front    : the waves sweep memory together (chunk = wave + k * 4096), 1 KB per instruction (16 B / lane) -- the ideal
//   streams  : every wave walks its OWN contiguous 1.2 MB region (= the records of one OCP instance), 1 KB per instruction
//   rows288  : own region, 288 B per instruction (36 lanes x 8 B: one column of Fxx / P per load, the forward kernel's)
// with U loads in flight per wave.  hipcc --offload-arch=gfx950 -O3 read_bw_probe.hip -o read_bw_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
typedef double d2 __attribute__((ext_vector_type(2)));
constexpr size_t REGION = 1216 * 1024;  // bytes per wave
constexpr int WAVES = 4096;

template <int U, bool FRONT>
__global__ __launch_bounds__(64) void read16(const char* __restrict__ base, double* out) {
  const int w = blockIdx.x, lane = threadIdx.x;
  constexpr int CH = REGION / 1024;  // 1 KB chunks per wave
  double acc = 0.0;
  for (int c = 0; c + U <= CH; c += U) {
    d2 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const size_t chunk = FRONT ? (size_t)w + (size_t)(c + k) * WAVES : (size_t)w * CH + (c + k);
      v[k] = *reinterpret_cast<const d2*>(base + chunk * 1024 + lane * 16);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) acc += v[k][0] + v[k][1];
  }
  if (acc == 1234.5) out[w] = acc;
}

template <int U>
__global__ __launch_bounds__(64) void read288(const char* __restrict__ base, double* out) {
  const int w = blockIdx.x, lane = threadIdx.x;
  constexpr int CH = REGION / 288;
  const char* p = base + (size_t)w * REGION + (lane < 36 ? lane : 0) * 8;
  double acc = 0.0;
  for (int c = 0; c + U <= CH; c += U) {
    double v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = *reinterpret_cast<const double*>(p + (size_t)(c + k) * 288);
#pragma unroll
    for (int k = 0; k < U; ++k) acc += v[k];
  }
  if (acc == 1234.5) out[w] = acc;
}

// ---- the forward kernel's matrix walk and its reduced forms (profiles/r11_symmetric_reads.txt).  Every wave walks MATS
//      36 x 36 column-major matrices (10,368 B each) out of its own region, MU matrices in flight, eight waves per CU like the
//      kernel (20 KB of dynamic LDS per block).  Loads are raw buffer loads of 16 B through a descriptor over the wave's region:
//      a silent lane's offset lies past num_records, so the range check drops its request (and nothing can leave the region).
//        PAIRS864 : lane c 18 + p reads rows 2p, 2p+1 of column 3t + c; 54 lanes, 12 loads per matrix (lanes 54.. repeat group 0)
//        TAILS    : the same map, lanes whose pair lies wholly above the diagonal (2p + 1 < column) silent: 342 of 648 pairs
//        HALVES   : the same map, row pairs 0..8 silent (rows 18..35 of every column)
//        HALVES7  : 9 row pairs x 7 column groups, lane c 9 + p reads rows 18 + 2p, 19 + 2p of column 7t + c; 6 loads per matrix
//        PAIRS864G: PAIRS864 with plain global loads, the kernel's own instruction ----
enum { PAIRS864 = 0, TAILS = 1, HALVES = 2, HALVES7 = 3, PAIRS864G = 4 };
constexpr int MAT = 36 * 36 * 8;
constexpr int MATS = REGION / MAT;  // 120
typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <int MODE, int MU>
__global__ __launch_bounds__(64) void readmat(const char* __restrict__ base, double* out) {
  extern __shared__ char occupancy_pad[];
  const int w = blockIdx.x, lane = threadIdx.x;
  const char* reg = base + (size_t)w * REGION;
  constexpr unsigned SILENT = 0x80000000u;
  constexpr bool SEVEN = MODE == HALVES7;
  constexpr int TL = SEVEN ? 6 : 12;
  const bool lg = lane < (SEVEN ? 63 : 54);
  const int p = SEVEN ? (lg ? lane % 9 : 0) : (lg ? lane % 18 : lane - 54);
  const int c = SEVEN ? (lg ? lane / 9 : 0) : (lg ? lane / 18 : 0);
  const unsigned lo = SEVEN ? c * 288 + 144 + 16 * p : c * 288 + 16 * p;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reg), 0, MATS * MAT, 0x00020000);
  unsigned acc = 0;
  for (int m = 0; m + MU <= MATS; m += MU) {
    u4 v[MU][TL];
#pragma unroll
    for (int k = 0; k < MU; ++k)
#pragma unroll
      for (int t = 0; t < TL; ++t) {
        const int col = (SEVEN ? 7 : 3) * t + c;
        bool live = true;
        if (MODE == TAILS) live = 2 * p + 1 >= col;
        if (MODE == HALVES) live = p >= 9;
        if (MODE == HALVES7) live = col < 36 && lg;
        const unsigned off = lo + (unsigned)((m + k) * MAT + t * (SEVEN ? 7 : 3) * 288);
        if (MODE == PAIRS864G)
          v[k][t] = *reinterpret_cast<const u4*>(reg + off);
        else
          v[k][t] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, live ? off : SILENT, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);   // every load of the MU matrices in flight before the first is consumed
#pragma unroll
    for (int k = 0; k < MU; ++k)
#pragma unroll
      for (int t = 0; t < TL; ++t) acc ^= v[k][t].x ^ v[k][t].y ^ v[k][t].z ^ v[k][t].w;
  }
  if (acc == 0x12345u) out[w] = acc + occupancy_pad[lane];
}

template <class F>
static void run(const char* name, double bytes, F launch) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  launch();
  hipDeviceSynchronize();
  float best = 1e30f, sum = 0.f;
  const int reps = 6;
  for (int r = 0; r < reps; ++r) {
    hipEventRecord(e0);
    launch();
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    best = ms < best ? ms : best;
    sum += ms;
  }
  printf("%-28s %7.3f ms (best %7.3f)  %6.2f TB/s (best %6.2f)\n", name, sum / reps, best, bytes / (sum / reps) * 1e-9,
         bytes / best * 1e-9);
}

// `read_bw_probe mats [rounds]`: the matrix walks, every variant once per round in interleaved order; per variant the median,
// fastest and slowest round as ns per matrix and wave.  Under a counter pass the dispatches are told apart by kernel name.
static int run_mats(const char* buf, double* out, int rounds) {
  struct V { const char* name; void (*kern)(const char*, double*); double req; };
  const V vs[] = {
      {"pairs864  (buffer loads)", readmat<PAIRS864, 2>, 648 * 16.0}, {"tails     342 of 648 pairs", readmat<TAILS, 2>, 342 * 16.0},
      {"halves    present map", readmat<HALVES, 2>, 324 * 16.0},      {"halves7   9 x 7 map", readmat<HALVES7, 2>, 324 * 16.0},
      {"halves7   4 in flight", readmat<HALVES7, 4>, 324 * 16.0},     {"pairs864g (global loads)", readmat<PAIRS864G, 2>, 648 * 16.0}};
  constexpr int NVAR = sizeof(vs) / sizeof(vs[0]);
  rounds = rounds < 1 ? 1 : (rounds > 64 ? 64 : rounds);
  static float ms[NVAR][64];
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int r = -1; r < rounds; ++r)   // round -1 warms up
    for (int i = 0; i < NVAR; ++i) {
      hipEventRecord(e0);
      vs[i].kern<<<WAVES, 64, 20480>>>(buf, out);
      hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) return 1;
      if (r >= 0) hipEventElapsedTime(&ms[i][r], e0, e1);
    }
  printf("%d waves x %d matrices of 36 x 36 doubles, %d rounds interleaved; ns per matrix and wave\n", WAVES, MATS, rounds);
  for (int i = 0; i < NVAR; ++i) {
    std::sort(ms[i], ms[i] + rounds);
    const double k = 1e6 / ((double)WAVES * MATS);
    printf("%-28s requested %6.0f B  median %7.3f  min %7.3f  max %7.3f  (%.3f ms per launch)\n", vs[i].name, vs[i].req,
           ms[i][rounds / 2] * k, ms[i][0] * k, ms[i][rounds - 1] * k, ms[i][rounds / 2]);
  }
  return 0;
}

int main(int argc, char** argv) {
  const size_t total = REGION * WAVES;
  char* buf;
  double* out;
  if (hipMalloc(&buf, total) != hipSuccess || hipMalloc(&out, WAVES * 8) != hipSuccess) return 1;
  hipMemset(buf, 0, total);
  if (argc > 1 && !strcmp(argv[1], "mats")) return run_mats(buf, out, argc > 2 ? atoi(argv[2]) : 9);
  const double B = (double)total;
#define R16(U, FRONT, NAME) run(NAME, B, [&] { read16<U, FRONT><<<WAVES, 64>>>(buf, out); })
#define R288(U, NAME) run(NAME, B, [&] { read288<U><<<WAVES, 64>>>(buf, out); })
  printf("%d waves x %zu KB = %.2f GB per launch\n", WAVES, REGION / 1024, B * 1e-9);
  R16(4, true, "front   1KB/instr  U=4");
  R16(8, true, "front   1KB/instr  U=8");
  R16(16, true, "front   1KB/instr  U=16");
  R16(4, false, "streams 1KB/instr  U=4");
  R16(8, false, "streams 1KB/instr  U=8");
  R16(16, false, "streams 1KB/instr  U=16");
  R16(32, false, "streams 1KB/instr  U=32");
  R288(8, "rows288 288B/instr U=8");
  R288(16, "rows288 288B/instr U=16");
  R288(32, "rows288 288B/instr U=32");
  R288(48, "rows288 288B/instr U=48");
  return 0;
}
