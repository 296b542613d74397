// mission.hip -- the goal source of the reference's mission layer on the device, one drone per lane:
// GlobalMissionPlanner.get_current_goal (src/dart_planner/planning/global_mission_planner.py:182-224, "mission.py"), the call that produces
// the goal every planner entry point reads, with its phase machine (mission_step of mission_device.hpp) and the stamp its global planning
// step makes on the UncertaintyField, as a row of the table se3mpc_ufield_stamp takes.
//
//   * get_current_goal             mission.py:182-224   se3mpc_mission_goal_*
//   * __init__ / the fresh record  mission.py:94-97, :156   se3mpc_mission_reset
//
// Contraction is off in this file: every threshold of the phase machine compares against values NumPy forms without FMA.
#pragma clang fp contract(off)
#include "mission_device.hpp"

namespace se3mpc {

__global__ void __launch_bounds__(256)
mission_reset_kernel(int B, double* __restrict__ state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* s = state + (size_t)b * SE3MPC_MISSION_STATE_WORDS;
  s[0] = (double)SE3MPC_MISSION_TAKEOFF;                                           // mission.py:95
  s[1] = 0.0;                                                                      // :97
  s[2] = 0.0;                                                                      // :156
  s[3] = 0.0;
}

template <typename IO>
__global__ void __launch_bounds__(256)
mission_goal_kernel(se3mpc_mission_params mp, int rv, int B, const double* __restrict__ now, const IO* __restrict__ pos, double* __restrict__ state,
                    MissionTable t, IO* __restrict__ goal, double* __restrict__ centres, double* __restrict__ radius,
                    int32_t* __restrict__ radius_voxels, double* __restrict__ factor) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double p[3] = {(double)pos[3 * (size_t)b], (double)pos[3 * (size_t)b + 1], (double)pos[3 * (size_t)b + 2]};
  double rec[SE3MPC_MISSION_STATE_WORDS];
  for (int i = 0; i < SE3MPC_MISSION_STATE_WORDS; ++i) rec[i] = state[(size_t)b * SE3MPC_MISSION_STATE_WORDS + i];
  double g[3];
  MissionStamp st;
  mission_step(mp, rv, now[b], p, rec, mission_rows(t, b), mission_labels(t, b), t.W, g, st);
  for (int i = 0; i < SE3MPC_MISSION_STATE_WORDS; ++i) state[(size_t)b * SE3MPC_MISSION_STATE_WORDS + i] = rec[i];
  for (int a = 0; a < 3; ++a) {
    goal[3 * (size_t)b + a] = (IO)g[a];                                            // rounded to the IO type once, here
    centres[3 * (size_t)b + a] = st.centre[a];
  }
  radius[b] = st.radius;
  radius_voxels[b] = st.radius_voxels;
  factor[b] = st.factor;
}

template <typename IO>
int mission_goal_impl(const se3mpc_mission_params* mp, int B, const double* now, const IO* pos, double* state, const double* waypoints,
                      long long wp_stride, const int32_t* labels, long long label_stride, int W, double resolution, IO* goal, double* centres,
                      double* radius, int32_t* radius_voxels, double* factor, void* stream) {
  if (mp == nullptr) return reject(SE3MPC_ERR_NULL, "se3mpc_mission_goal: params");
  const int rc = check_mission_params(mp);
  if (rc) return reject(rc, "se3mpc_mission_goal: a non-finite parameter or a period <= 0");
  if (B < 0 || B > (1 << 30)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_mission_goal: B outside [0, 2^30]");
  const MissionTable t = {waypoints, wp_stride, labels, label_stride, W};
  const int trc = check_mission_table(mp, t, resolution, "se3mpc_mission_goal: W < 0, a stride smaller than the table, or the resolution");
  if (trc) return trc;
  if (B == 0) return SE3MPC_OK;
  if (!now || !pos || !state || !goal || !centres || !radius || !radius_voxels || !factor || (W > 0 && (!waypoints || !labels)))
    return reject(SE3MPC_ERR_NULL, "se3mpc_mission_goal: now / pos / state / goal / the stamp table / the waypoint table");
  hipLaunchKernelGGL((mission_goal_kernel<IO>), dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, *mp, mission_radius_voxels(mp, resolution), B,
                     now, pos, state, t, goal, centres, radius, radius_voxels, factor);
  return launch_status("se3mpc_mission_goal");
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" int se3mpc_mission_default_params(se3mpc_mission_params* out) {
  if (out == nullptr) return SE3MPC_ERR_NULL;
  se3mpc_mission_params p;
  p.safe_altitude = 5.0;                    // mission.py:256
  p.takeoff_band = 0.5;                     // :261
  p.waypoint_reach = 2.0;                   // :322
  p.safety_margin = 2.0;                    // :48
  p.landing_pad_lift = 3.0;                 // :380
  p.landing_step = 1.0;                     // :347
  p.landing_floor = 0.5;
  p.emergency_step = 2.0;                   // :358
  p.emergency_floor = 0.0;
  p.emergency_altitude = 0.5;               // :454
  p.global_replan_period = 1.0 / 1.0;       // :60, :198
  p.exploration_base = 10.0;                // :284
  p.exploration_radius = 50.0;              // :46
  p.stamp_radius = 3.0;                     // :412
  p.stamp_factor = 0.2;
  p.use_neural_scene = 1;                   // :51
  p.reserved = 0;
  *out = p;
  return SE3MPC_OK;
}

extern "C" int se3mpc_check_mission_params(const se3mpc_mission_params* mp) { return check_mission_params(mp); }

extern "C" int se3mpc_mission_reset(int B, double* state, void* stream) {
  if (B < 0) return SE3MPC_ERR_SHAPE;
  if (B == 0) return SE3MPC_OK;
  if (state == nullptr) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(mission_reset_kernel, dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, B, state);
  return launch_status("se3mpc_mission_reset");
}

extern "C" int se3mpc_mission_goal_f32(const se3mpc_mission_params* mp, int B, const double* now, const float* pos, double* mission_state,
                                       const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride, int W,
                                       double resolution, float* goal, double* stamp_centres, double* stamp_radius, int32_t* stamp_radius_voxels,
                                       double* stamp_factor, void* stream) {
  return mission_goal_impl<float>(mp, B, now, pos, mission_state, waypoints, wp_stride, labels, label_stride, W, resolution, goal, stamp_centres,
                                  stamp_radius, stamp_radius_voxels, stamp_factor, stream);
}
extern "C" int se3mpc_mission_goal_f64(const se3mpc_mission_params* mp, int B, const double* now, const double* pos, double* mission_state,
                                       const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride, int W,
                                       double resolution, double* goal, double* stamp_centres, double* stamp_radius, int32_t* stamp_radius_voxels,
                                       double* stamp_factor, void* stream) {
  return mission_goal_impl<double>(mp, B, now, pos, mission_state, waypoints, wp_stride, labels, label_stride, W, resolution, goal, stamp_centres,
                                   stamp_radius, stamp_radius_voxels, stamp_factor, stream);
}
