// TEST INFRASTRUCTURE ONLY -- the emulator's launch record (see hip_emu.h). With EMU_PLAN_TRACE=<file> set, every kernel
// launch of the emulator build appends one line: the kernel instantiation as the launch macro names it, the grid, the
// block and the dynamic LDS bytes -- in plan-only mode (EMU_PLAN_ONLY=1) as well as when kernels execute. The variable is
// read once per process. scripts/launch_plan.py and tests/test_launch_plan_emu.py read the file.
#pragma once
#include "hip_emu.h"

namespace emu {
inline void plan_trace(const char* kernel, dim3 grid, dim3 block, size_t smem) {
  static FILE* const f = [] { const char* t = getenv("EMU_PLAN_TRACE"); return t && *t ? fopen(t, "a") : (FILE*)nullptr; }();
  if (!f) return;
  fprintf(f, "%s grid=%u,%u,%u block=%u,%u,%u lds=%zu\n", kernel, grid.x, grid.y, grid.z, block.x, block.y, block.z, smem);
  fflush(f);
}
}  // namespace emu
