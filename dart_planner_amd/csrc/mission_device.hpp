// mission_device.hpp -- GlobalMissionPlanner.get_current_goal for one drone, shared by mission.hip (one drone per lane) and
// monte_carlo_mission.hip (the group's first lane, at the head of every planning cycle).
// INCLUDE UNDER `#pragma clang fp contract(off)`: the takeoff altitude, the reach distance, the emergency altitude and the replan gate
// compare against values NumPy forms one rounded operation at a time.
//
// Reference arithmetic ("mission.py" = src/dart_planner/planning/global_mission_planner.py), unit-stripped and reproduced with its quirks.
// Not reproduced: the np.random parts (the simulated high-uncertainty regions of :433-442 and the placeholder of :462-465, which only the
// non-empty branch of _plan_exploration_goal reads) and PlaceholderNeuralScene (its update count is the record's plan count).
#pragma once
#pragma clang fp contract(off)

#include <cmath>

#include "se3mpc_common.hpp"

static_assert(sizeof(se3mpc_mission_params) == 128, "se3mpc_mission_params is part of the C ABI (capi.MissionParams mirrors it)");

namespace se3mpc {

// The waypoint table of the C ABI as one kernel argument: W rows, positions [W][3] and labels [W] with the strides in elements from drone
// to drone (0: one table shared by all).
struct MissionTable {
  const double* wp; long long wp_stride;
  const int32_t* label; long long label_stride;
  int W;
};

// One row of the stamp table se3mpc_ufield_stamp reads (radius_voxels < 0: nothing stamped)
struct MissionStamp {
  double centre[3], radius, factor;
  int32_t radius_voxels;
};

// a record word as a small integer: NaN and everything below 0 read as 0
__host__ __device__ __forceinline__ int mission_word(double v, int top) { return v >= 0.0 ? (v > (double)top ? top : (int)v) : 0; }

// max(a, b) as Python evaluates it: a unless b > a (a NaN b never wins)
__host__ __device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// get_current_goal (mission.py:182-224) on the record rec [SE3MPC_MISSION_STATE_WORDS] at position p and wall clock `now`.  rv = int(radius /
// resolution) of the stamp, computed once by the host.  -> goal[3] in double and the stamp row of this call.
__host__ __device__ __forceinline__ void mission_step(const se3mpc_mission_params& mp, int rv, double now, const double p[3], double* rec,
                                                      const double* __restrict__ wp, const int32_t* __restrict__ label, int W, double goal[3],
                                                      MissionStamp& stamp) {
  const double pw = rec[0];
  int phase = (pw >= 0.0 && pw <= (double)SE3MPC_MISSION_EMERGENCY) ? (int)pw : -1;    // anything else: mission.py:222-224
  int idx = mission_word(rec[1], 1 << 30);
  for (int a = 0; a < 3; ++a) stamp.centre[a] = p[a];
  stamp.radius = -1.0; stamp.radius_voxels = -1; stamp.factor = mp.stamp_factor;
  if (now - rec[2] > mp.global_replan_period) {                                        // :195-201
    if (mp.use_neural_scene) { stamp.radius = mp.stamp_radius; stamp.radius_voxels = rv; }   // :409-413
    if (p[2] < mp.emergency_altitude && phase != SE3MPC_MISSION_LANDING) phase = SE3MPC_MISSION_EMERGENCY;   // :450-458
    rec[3] = rec[3] + 1.0;
    rec[2] = now;
  }
  goal[0] = p[0]; goal[1] = p[1]; goal[2] = p[2];
  if (phase == SE3MPC_MISSION_TAKEOFF) {                                               // :254-265
    goal[2] = mp.safe_altitude;
    if (p[2] >= mp.safe_altitude - mp.takeoff_band) phase = SE3MPC_MISSION_NAVIGATION;
  } else if (phase == SE3MPC_MISSION_EXPLORATION) {                                    // :279-294, no region, nothing explored: angle 0
    const double radius = mp.exploration_radius < mp.exploration_base ? mp.exploration_radius : mp.exploration_base;
    goal[0] = p[0] + radius * 1.0;
    goal[1] = p[1] + radius * 0.0;
  } else if (phase == SE3MPC_MISSION_NAVIGATION || phase == SE3MPC_MISSION_MAPPING) {  // :296-341
    if (W > 0) {
      bool done = idx >= W;                                                            // :310-313
      if (!done) {
        const double* w = wp + 3 * (size_t)idx;
        const double dx = p[0] - w[0], dy = p[1] - w[1], dz = p[2] - w[2];
        if (sqrt((dx * dx + dy * dy) + dz * dz) < mp.waypoint_reach) {                 // :318-326
          idx += 1;
          done = idx >= W;                                                             // :329-331
        }
      }
      if (done) {
        phase = SE3MPC_MISSION_LANDING;
      } else {                                                                         // _apply_semantic_reasoning, :362-386
        const double* w = wp + 3 * (size_t)idx;
        const int lab = label[idx];
        goal[0] = w[0]; goal[1] = w[1]; goal[2] = w[2];
        if (lab == SE3MPC_LABEL_OBSTACLE) {
          const double d[3] = {p[0] - w[0], p[1] - w[1], p[2] - w[2]};
          const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
          if (n > 0.0)
            for (int a = 0; a < 3; ++a) goal[a] = w[a] + (d[a] / n) * mp.safety_margin;
        } else if (lab == SE3MPC_LABEL_LANDING_PAD) {
          goal[2] = py_max(w[2] + mp.landing_pad_lift, p[2]);
        }
      }
    }
  } else if (phase == SE3MPC_MISSION_LANDING) {                                        // :343-353
    goal[2] = py_max(mp.landing_floor, p[2] - mp.landing_step);
  } else if (phase == SE3MPC_MISSION_EMERGENCY) {                                      // :355-360
    goal[2] = py_max(mp.emergency_floor, p[2] - mp.emergency_step);
  }
  if (phase >= 0) rec[0] = (double)phase;
  rec[1] = (double)idx;
}

// drone b's rows of the table (W = 0: nothing is read)
__host__ __device__ __forceinline__ const double* mission_rows(const MissionTable& t, int b) {
  return t.W > 0 ? t.wp + (size_t)b * t.wp_stride : nullptr;
}
__host__ __device__ __forceinline__ const int32_t* mission_labels(const MissionTable& t, int b) {
  return t.W > 0 ? t.label + (size_t)b * t.label_stride : nullptr;
}

inline int check_mission_params(const se3mpc_mission_params* mp) {
  if (mp == nullptr) return SE3MPC_ERR_NULL;
  const double* d = reinterpret_cast<const double*>(mp);
  for (int i = 0; i < 15; ++i)
    if (!std::isfinite(d[i])) return SE3MPC_ERR_PARAM;
  if (!(mp->global_replan_period > 0.0)) return SE3MPC_ERR_PARAM;
  return SE3MPC_OK;
}

// The rules every entry point with a waypoint table shares: W >= 0, strides 0 or at least a table: SE3MPC_ERR_SHAPE; a resolution that is not
// finite and positive when stamps are made: SE3MPC_ERR_PARAM.  Presence (W > 0: both tables) is asked after the B == 0 no-op.
inline int check_mission_table(const se3mpc_mission_params* mp, const MissionTable& t, double resolution, const char* what) {
  if (t.W < 0 || t.W > (1 << 20) || !(t.wp_stride == 0 || t.wp_stride >= 3LL * t.W) || !(t.label_stride == 0 || t.label_stride >= (long long)t.W))
    return reject(SE3MPC_ERR_SHAPE, what);
  if (mp->use_neural_scene && !(resolution > 0.0 && std::isfinite(resolution))) return reject(SE3MPC_ERR_PARAM, what);
  return SE3MPC_OK;
}

// int(radius / resolution) as Python's float64 gives it (field.py:234), kept inside an int
inline int mission_radius_voxels(const se3mpc_mission_params* mp, double resolution) {
  if (!mp->use_neural_scene) return -1;
  const double q = mp->stamp_radius / resolution;
  return q >= 1073741824.0 ? (1 << 30) : (q <= -1.0 ? -1 : (int)q);
}

}  // namespace se3mpc
