// robotoc::BipedWalkFootStepPlanner (robotoc_amd/host/robotoc_hip_planner.hpp) over the C ABI: a batch of iCubs, every one with its
// own step length and yaw, planned on the device through the header class (setGaitPattern, init, plan, place) and read back.
// tests/test_cpp_biped_walk_foot_step_planner.py compares the plan with the numpy restatement of the reference and the two placement
// tables with the plan.
//   usage: biped_walk_foot_step_planner_test <problem.bin> <out.bin>
//   problem.bin: as tests/cpp/foot_step_planner_test.cpp -- rtoc_dims | int n | rtoc_grid[n] | rtoc_robot_model | int batch |
//                x0[batch][nq + nv] | step_length[batch][3] | step_yaw[batch] | int phase[n] | unsigned masks[n] | int planning_steps
//   the walk plans with double support at 0b11 and then at 0b01 (the right foot swings)
//   out.bin (doubles): size, current_step, positions[batch][size][2][3], surfaces[batch][size][2][9], com[batch][size][3],
//                R[batch][size][9], ok[batch], table positions[batch][n][2][3], table rotations[batch][n][2][9], per_instance
#include <cstdio>
#include <cstring>
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
    BipedWalkFootStepPlanner planner(ctx, batch, RTOC_PROJECT_YAW);
    // the setters refuse what the reference's refuse (:66-74), and a command of the wrong size
    int refused = 0;
    try {
      planner.setGaitPattern(std::vector<double>(4, 0.0), yaw, false);   // neither 3 nor 3 per instance
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    const std::vector<double> v3(3, 0.0), y1(1, 0.0);
    const double bad[3][3] = {{0.0, 0.1, 0.7}, {0.2, -0.1, 0.7}, {0.2, 0.1, 0.0}};   // swing_time, double_support_time, gain
    for (const auto& t : bad) {
      try {
        planner.setRaibertGaitPattern(v3, y1, t[0], t[1], t[2]);
      } catch (const std::out_of_range&) {
        ++refused;
      }
    }
    if (refused != 4) return 8;
    planner.setRaibertGaitPattern(v3, y1, 0.2, 0.0, 0.7);   // no double support: allowed
    planner.setGaitPattern(sl, yaw, true);
    planner.init();
    if (planner.size() != 0) return 9;
    if (planner.plan(0.0, 0x0u, steps) || planner.plan(0.0, 0x7u, steps) || planner.plan(0.0, 0x9u, steps)) return 9;   // false, as the reference
    if (!planner.plan(0.0, 0x3u, steps) || !planner.plan(0.1, 0x1u, steps)) return 9;
    planner.place(phase);
    const int size = planner.size();
    std::vector<double> out;
    out.push_back(size), out.push_back(planner.currentStep());
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.contactPositions(b, s), planner.contactPositions(b, s) + 6);
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) {
        // contactSurfaces(step) and contactPlacements(step) name the same rotations, and the placements the same translations
        const auto pl = planner.contactPlacements(b, s);
        const double* const S = planner.contactSurfaces(b, s);
        if (pl[0].rotation != S || pl[1].rotation != S + 9 || pl[0].translation != planner.contactPositions(b, s) ||
            pl[1].translation != planner.contactPositions(b, s) + 3)
          return 10;
        out.insert(out.end(), S, S + 18);
      }
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.CoM(b, s), planner.CoM(b, s) + 3);
    for (int b = 0; b < batch; ++b)
      for (int s = 0; s < size; ++s) out.insert(out.end(), planner.R(b, s), planner.R(b, s) + 9);
    for (int b = 0; b < batch; ++b) out.push_back(planner.ok(b) ? 1.0 : 0.0);
    std::vector<double> tab_p((size_t)batch * n * 6), tab_r((size_t)batch * n * 18);
    int inst = 0;
    if (rtoc_get_contact_placements(ctx, tab_p.data(), tab_r.data(), batch, &inst) != RTOC_OK) throw std::runtime_error("rtoc_get_contact_placements");
    out.insert(out.end(), tab_p.begin(), tab_p.end());
    out.insert(out.end(), tab_r.begin(), tab_r.end());
    out.push_back(inst);
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("biped walk planner on the device: %d instances, plan of %d steps, placements per instance %d\n", batch, size, inst);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    rtoc_destroy(ctx);
    return 7;
  }
  rtoc_destroy(ctx);
  return 0;
}
