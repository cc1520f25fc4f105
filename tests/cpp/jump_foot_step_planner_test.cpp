// robotoc::JumpFootStepPlanner (robotoc_amd/host/robotoc_hip_planner.hpp) over the C ABI: a batch of robots, every one with its own
// jump length and yaw, planned on the device through the header class (setJumpPattern, init, resetContactPlacements,
// setConfigurationRef) and read back.  tests/test_cpp_jump_foot_step_planner.py compares everything with the Python shell's read-back
// of the same calls.
//   usage: jump_foot_step_planner_test <problem.bin> <out.bin>
//   problem.bin: rtoc_dims | int n | rtoc_grid[n] | rtoc_robot_model | int batch | x0[batch][nq + nv] | jump_length[batch][3] |
//                step_yaw[batch] | int phase[n] | unsigned masks[n] | x1[batch][nq + nv]
//   the jump is initialised at x0, ticks on the ground (every contact) at x0, then in the air (no contact) at x1
//   out.bin (doubles), once per tick: size, current_step, positions[batch][size][nf][3], surfaces[batch][size][nf][9],
//                com[batch][size][3], R[batch][size][9], ok[batch], jump_length[batch][3], table positions[batch][n][nf][3],
//                table rotations[batch][n][nf][9], per_instance, q_ref table[batch][n][nq], active[batch][n]
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
  int n = 0, batch = 0;
  if (!rd(f, &dims, 1) || !rd(f, &n, 1) || n < 2) return 4;
  std::vector<rtoc_grid> grid(n);
  if (!rd(f, grid.data(), n) || !rd(f, &model, 1) || !rd(f, &batch, 1) || batch < 1) return 4;
  const int nx = model.nq + model.nv, nf = model.ncontacts, nq = model.nq;
  std::vector<double> x0((size_t)batch * nx), x1((size_t)batch * nx), jl((size_t)batch * 3), yaw(batch);
  std::vector<int> phase(n);
  std::vector<unsigned> masks(n);
  if (!rd(f, x0.data(), x0.size()) || !rd(f, jl.data(), jl.size()) || !rd(f, yaw.data(), yaw.size()) || !rd(f, phase.data(), n) ||
      !rd(f, masks.data(), n) || !rd(f, x1.data(), x1.size()))
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
    int refused = 0;
    try {
      JumpFootStepPlanner three(ctx, batch, 3);   // neither a quadruped nor a biped
    } catch (const std::out_of_range&) {
      ++refused;
    }
    JumpFootStepPlanner planner(ctx, batch, nf, RTOC_PROJECT_YAW);
    try {
      planner.setJumpPattern(std::vector<double>(4, 0.0), yaw);   // neither 3 nor 3 per instance
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    if (refused != 2) return 8;
    planner.setJumpPattern(jl, yaw);
    planner.init();
    if (planner.size() != 3 || planner.currentStep() != 0) return 9;   // MPCJump::init reads CoM(2) and R(2) before it plans
    const unsigned full = (1u << nf) - 1u;
    if (planner.plan(0.0, full + 1u)) return 9;   // a contact the model does not have: false
    std::vector<double> out;
    for (int tick = 0; tick < 2; ++tick) {
      if (tick == 1 && rtoc_set_initial_state(ctx, x1.data(), batch) != RTOC_OK) return 6;
      if (!resetContactPlacements(planner, 0.1 * tick, tick == 0 ? full : 0u, phase)) return 9;
      planner.setConfigurationRef(n);
      const int size = planner.size();
      out.push_back(size), out.push_back(planner.currentStep());
      for (int b = 0; b < batch; ++b)
        for (int s = 0; s < size; ++s) out.insert(out.end(), planner.contactPositions(b, s), planner.contactPositions(b, s) + 3 * nf);
      for (int b = 0; b < batch; ++b)
        for (int s = 0; s < size; ++s) {
          // contactSurfaces(step) and contactPlacements(step) name the same rotations, and the placements the same translations
          const auto pl = planner.contactPlacements(b, s);
          const double* const S = planner.contactSurfaces(b, s);
          if ((int)pl.size() != nf) return 10;
          for (int k = 0; k < nf; ++k)
            if (pl[k].rotation != S + 9 * k || pl[k].translation != planner.contactPositions(b, s) + 3 * k) return 10;
          out.insert(out.end(), S, S + 9 * nf);
        }
      for (int b = 0; b < batch; ++b)
        for (int s = 0; s < size; ++s) out.insert(out.end(), planner.CoM(b, s), planner.CoM(b, s) + 3);
      for (int b = 0; b < batch; ++b)
        for (int s = 0; s < size; ++s) out.insert(out.end(), planner.R(b, s), planner.R(b, s) + 9);
      for (int b = 0; b < batch; ++b) out.push_back(planner.ok(b) ? 1.0 : 0.0);
      for (int b = 0; b < batch; ++b) out.insert(out.end(), planner.jumpLength(b), planner.jumpLength(b) + 3);
      std::vector<double> tab_p((size_t)batch * n * nf * 3), tab_r((size_t)batch * n * nf * 9), q_ref((size_t)batch * n * nq);
      std::vector<int> active((size_t)batch * n);
      int inst = 0, q_inst = 0;
      if (rtoc_get_contact_placements(ctx, tab_p.data(), tab_r.data(), batch, &inst) != RTOC_OK) throw std::runtime_error("rtoc_get_contact_placements");
      if (rtoc_get_configuration_ref_table(ctx, q_ref.data(), active.data(), batch, &q_inst) != RTOC_OK || q_inst != 1)
        throw std::runtime_error("rtoc_get_configuration_ref_table");
      out.insert(out.end(), tab_p.begin(), tab_p.end());
      out.insert(out.end(), tab_r.begin(), tab_r.end());
      out.push_back(inst);
      out.insert(out.end(), q_ref.begin(), q_ref.end());
      out.insert(out.end(), active.begin(), active.end());
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("jump planner on the device: %d instances on %d feet, two ticks\n", batch, nf);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    rtoc_destroy(ctx);
    return 7;
  }
  rtoc_destroy(ctx);
  return 0;
}
