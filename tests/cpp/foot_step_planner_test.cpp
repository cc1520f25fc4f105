// robotoc::TrotFootStepPlanner (robotoc_amd/host/robotoc_hip_planner.hpp) over the C ABI: a batch of ANYmals, every one with its own
// step length and yaw, planned on the device through the header class (setGaitPattern, init, plan, place) and read back.
// tests/test_cpp_foot_step_planner.py compares the plan with the numpy restatement of the reference and the placement table with
// the plan.
//   usage: foot_step_planner_test <problem.bin> <out.bin>
//   problem.bin: rtoc_dims | int n | rtoc_grid[n] | rtoc_robot_model | int batch | x0[batch][nq + nv] | step_length[batch][3] |
//                step_yaw[batch] | int phase[n] | unsigned masks[n] | int planning_steps
//   out.bin (doubles): size, current_step, positions[batch][size][12], com[batch][size][3], R[batch][size][9], ok[batch],
//                placements[batch][n][4][3], per_instance
#include <cstdio>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_planner.hpp"

using namespace robotoc;

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  rtoc_dims dims;
  rtoc_robot_model model;
  int n = 0, batch = 0, steps = 0;
  if (!rd(f, &dims, 1) || !rd(f, &n, 1) || n < 2) return 4;
  std::vector<rtoc_grid> grid(n);
  if (!rd(f, grid.data(), n) || !rd(f, &model, 1) || !rd(f, &batch, 1) || batch < 1) return 4;
  const int nx = model.nq + model.nv;
  std::vector<double> x0((size_t)batch * nx), sl((size_t)batch * 3), yaw(batch);
  std::vector<int> phase(n);
  std::vector<unsigned> masks(n);
  if (!rd(f, x0.data(), x0.size()) || !rd(f, sl.data(), sl.size()) || !rd(f, yaw.data(), yaw.size()) || !rd(f, phase.data(), n) ||
      !rd(f, masks.data(), n) || !rd(f, &steps, 1))
    return 4;
  std::fclose(f);
  rtoc_ctx* ctx = nullptr;
  if (rtoc_create(&dims, n, batch, 0, &ctx) != RTOC_OK) return 5;
  int rc = rtoc_set_grid(ctx, grid.data(), n);
  if (!rc) rc = rtoc_set_robot_model(ctx, &model);
  if (!rc) rc = rtoc_set_contact_schedule(ctx, masks.data(), nullptr, nullptr);
  if (!rc) rc = rtoc_set_initial_state(ctx, x0.data(), batch);
  if (rc) return 6;
  try {
    TrotFootStepPlanner planner(ctx, batch, RTOC_PROJECT_YAW);
    int refused = 0;
    try {
      planner.setGaitPattern(std::vector<double>(4, 0.0), yaw, false);   // neither 3 nor 3 per instance
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    try {
      planner.setRaibertGaitPattern(std::vector<double>(3, 0.0), std::vector<double>(1, 0.0), 0.0, 0.1, 0.7);   // swing_time
    } catch (const std::out_of_range&) {
      ++refused;
    }
    if (refused != 2) return 8;
    planner.setGaitPattern(sl, yaw, false);
    planner.init();
    if (planner.size() != 0) return 9;
    if (planner.plan(0.0, 0x3u, steps)) return 9;   // no trot stance: false, as the reference
    if (!planner.plan(0.0, 0xFu, steps)) return 9;
    planner.place(phase);
    const int size = planner.size();
    std::vector<double> out;
    out.push_back(size), out.push_back(planner.currentStep());
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.contactPositions(b, s), planner.contactPositions(b, s) + 12);
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.CoM(b, s), planner.CoM(b, s) + 3);
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.R(b, s), planner.R(b, s) + 9);
    for (int b = 0; b < batch; ++b) out.push_back(planner.ok(b) ? 1.0 : 0.0);
    std::vector<double> table((size_t)batch * n * 12);
    int inst = 0;
    if (rtoc_get_contact_placements(ctx, table.data(), nullptr, batch, &inst) != RTOC_OK) return 10;
    out.insert(out.end(), table.begin(), table.end());
    out.push_back(inst);
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("TrotFootStepPlanner on the device: %d instances, plan of %d steps, placements per instance %d\n", batch, size, inst);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    rtoc_destroy(ctx);
    return 7;
  }
  rtoc_destroy(ctx);
  return 0;
}
