// robotoc::CrawlFootStepPlanner and robotoc::FlyingTrotFootStepPlanner (robotoc_amd/host/robotoc_hip_planner.hpp) over the C ABI: a
// batch of ANYmals, every one with its own step length and yaw, planned on the device through the header classes (setGaitPattern,
// init, plan, place) and read back.  tests/test_cpp_gait_foot_step_planner.py compares the plan with the numpy restatement of the
// reference and the placement table with the plan.
//   usage: gait_foot_step_planner_test <problem.bin> <out.bin> crawl|flying_trot
//   problem.bin: as tests/cpp/foot_step_planner_test.cpp -- rtoc_dims | int n | rtoc_grid[n] | rtoc_robot_model | int batch |
//                x0[batch][nq + nv] | step_length[batch][3] | step_yaw[batch] | int phase[n] | unsigned masks[n] | int planning_steps
//   the crawl plans once, at the status 0b0111 with the stance phase; the flying trot plans at 0b1001 and then a flight
//   out.bin (doubles): size, current_step, positions[batch][size][12], com[batch][size][3], R[batch][size][9], ok[batch],
//                placements[batch][n][4][3], per_instance
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robotoc_amd/host/robotoc_hip_planner.hpp"

using namespace robotoc;

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

template <class Planner>
static void read_back(Planner& planner, rtoc_ctx* ctx, const int batch, const int n, std::vector<double>& out, int* inst) {
  const int size = planner.size();
  out.push_back(size), out.push_back(planner.currentStep());
  for (int b = 0; b < batch; ++b)
    for (int s = 0; s < size; ++s) out.insert(out.end(), planner.contactPositions(b, s), planner.contactPositions(b, s) + 12);
  for (int b = 0; b < batch; ++b)
    for (int s = 0; s < size; ++s) out.insert(out.end(), planner.CoM(b, s), planner.CoM(b, s) + 3);
  for (int b = 0; b < batch; ++b)
    for (int s = 0; s < size; ++s) out.insert(out.end(), planner.R(b, s), planner.R(b, s) + 9);
  for (int b = 0; b < batch; ++b) out.push_back(planner.ok(b) ? 1.0 : 0.0);
  std::vector<double> table((size_t)batch * n * 12);
  if (rtoc_get_contact_placements(ctx, table.data(), nullptr, batch, inst) != RTOC_OK) throw std::runtime_error("rtoc_get_contact_placements");
  out.insert(out.end(), table.begin(), table.end());
  out.push_back(*inst);
}

// the setters refuse what the reference's refuse: a command of the wrong size, a time in the air that is not positive
template <class Planner, class Fixed>
static int refusals(Planner& planner, Fixed set_fixed_of_four) {
  int refused = 0;
  try {
    set_fixed_of_four();   // neither 3 nor 3 per instance
  } catch (const std::invalid_argument&) {
    ++refused;
  }
  try {
    planner.setRaibertGaitPattern(std::vector<double>(3, 0.0), std::vector<double>(1, 0.0), 0.0, 0.1, 0.7);
  } catch (const std::out_of_range&) {
    ++refused;
  }
  return refused;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool crawl = std::strcmp(argv[3], "crawl") == 0;
  if (!crawl && std::strcmp(argv[3], "flying_trot") != 0) return 2;
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
    std::vector<double> out;
    int inst = 0, size = 0;
    if (crawl) {
      CrawlFootStepPlanner planner(ctx, batch, RTOC_PROJECT_YAW);
      if (refusals(planner, [&] { planner.setGaitPattern(std::vector<double>(4, 0.0), yaw, false); }) != 2) return 8;
      planner.setGaitPattern(sl, yaw, true);
      planner.init();
      if (planner.size() != 0) return 9;
      if (planner.plan(0.0, 0x9u, steps) || planner.plan(0.0, 0x0u, steps)) return 9;   // no crawl stance: false, as the reference
      if (!planner.plan(0.0, 0x7u, steps)) return 9;
      planner.place(phase);
      read_back(planner, ctx, batch, n, out, &inst);
      size = planner.size();
    } else {
      FlyingTrotFootStepPlanner planner(ctx, batch, RTOC_PROJECT_YAW);
      if (refusals(planner, [&] { planner.setGaitPattern(std::vector<double>(4, 0.0), yaw); }) != 2) return 8;
      try {
        planner.setRaibertGaitPattern(std::vector<double>(3, 0.0), std::vector<double>(1, 0.0), 0.1, 0.0, 0.7);   // stance_time
        return 8;
      } catch (const std::out_of_range&) {
      }
      planner.setGaitPattern(sl, yaw);
      planner.init();
      if (planner.size() != 0) return 9;
      if (planner.plan(0.0, 0x3u, steps) || planner.plan(0.0, 0x7u, steps)) return 9;   // no flying-trot status
      try {
        planner.plan(0.0, 0x0u, steps);   // a flight with no plan behind it: the library refuses
        return 9;
      } catch (const std::runtime_error&) {
      }
      if (!planner.plan(0.0, 0x9u, steps) || !planner.plan(0.1, 0x0u, steps)) return 9;
      planner.place(phase);
      read_back(planner, ctx, batch, n, out, &inst);
      size = planner.size();
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    std::printf("%s planner on the device: %d instances, plan of %d steps, placements per instance %d\n", argv[3], batch, size, inst);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    rtoc_destroy(ctx);
    return 7;
  }
  rtoc_destroy(ctx);
  return 0;
}
