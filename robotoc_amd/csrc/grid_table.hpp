// grid_table.hpp -- a device table with one row per grid point that the batch shares or every instance has its own of (host side
// only; DevBuf one level up): the contact placements, the q_ref table, the reference tables of the task-space terms.  Invariants
// (DESIGN.md 1): a new capacity is staged beside the table in force and replaces it only at commit (the halves of a pair are both
// staged, then both committed), so a failed hipMalloc changes nothing; nstages is the grid the rows were set for (0: none, or
// forgotten), a per-instance table being [batch][nstages][row] whatever the capacity; per_instance is how the rows in force are
// laid out, not how large the allocation is.  No launches, no argument blocks: the launchers read buf.p, nstages, per_instance.
#pragma once
#include <cstring>

#include "device_buffer.hpp"

namespace rtoc {

template <class T>
struct GridTable {
  DevBuf<T> buf;
  int nstages = 0, per_instance = 0;
  int on = 0;         // the launchers read the table: a q_ref table is in use (kept across forget), placements were given
  DevBuf<T> staged;   // between stage and commit: the replacement of buf

  // `capacity` elements to fill (target) ahead of commit; 0: this call brings no rows.  in_place = false: the rows in force are
  // read while the new ones are written.  hipMalloc synchronises the device
  hipError_t stage(size_t capacity, bool in_place = true) {
    staged.release();
    return (capacity == 0 || (in_place && buf.p && buf.n == capacity)) ? hipSuccess : staged.reserve(capacity);
  }
  T* target() const { return staged.p ? staged.p : buf.p; }
  // true: something a launcher reads changed (pointer, mode, grid, on / off) and is baked into captured graphs -- the caller
  // starts a new epoch; false: the same table set again in place
  bool commit(int n, int inst, int use = 1) {
    const bool changed = staged.p || n != nstages || inst != per_instance || use != on;
    if (staged.p) buf = std::move(staged);
    nstages = n, per_instance = inst, on = use;
    return changed;
  }
  bool in_force(int n) const { return on && buf.p && nstages == n; }
  T* rows() const { return on ? buf.p : nullptr; }
  void forget() { nstages = 0; }   // the grid is gone (on stays: a table in use never gives way to a constant silently)
  // the table of `count` instances as they read it, a shared one repeated; row: elements per grid point
  hipError_t download(T* host, size_t row, int count, hipStream_t s) const {
    const size_t n = (size_t)nstages * row;
    if (!host || count < 1 || n == 0) return hipSuccess;
    hipError_t e = hipMemcpyAsync(host, buf.p, sizeof(T) * n * (per_instance ? count : 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (int b = 1; e == hipSuccess && !per_instance && b < count; ++b) memcpy(host + b * n, host, sizeof(T) * n);
    return e;
  }
  template <class Dup>   // rtoc_clone (Dup: CopyChain of rt_context.hpp): the allocation and what is known about it, together
  void clone_from(const GridTable& src, Dup& dup) {
    dup(buf, src.buf);
    nstages = src.nstages, per_instance = src.per_instance, on = src.on;
  }
};

}  // namespace rtoc
