// step_dispatch.hpp -- which of the step-kernel instantiations of step_instances.hpp a step call launches: the choice as a
// pure function of the facts it depends on (select_step_instance: tests/test_step_dispatch.py holds it to a restatement
// of its rules, over the whole grid of facts), and the chosen instantiation handed to a launch as compile-time
// constants (with_step_instance, in the style of for_mlp_instance of mlp_instances.hpp). Host code only: no HIP call, no handle.
#pragma once

#include <type_traits>

#include "step_kernels.hpp"

namespace upkie {

// 256 CUs x 4 SIMDs x 64 lanes x 2 waves
static const int kDenseBatch = 131072;
// up to this many envs two lanes per env still fit one wave per SIMD (1024 SIMDs x 64 lanes / 2)
static const int kPairBatch = 32768;

// up to this many envs the eight-lane kernel (step_kernel_octet) is at least as fast as the two-lane one: one wave per
// SIMD up to 8192 envs (16.5 us), two from there to 16384, where both mappings take 25.3 us -- the two co-resident
// waves do overlap, but the SIMD's issue port is then busy for the whole launch (profiles/r03_two_waves_per_simd_pmc.json)
// -- and the eight-lane kernel is the one that can carry the MPC balancer (upkie_sim_step_base_velocity_mpc) and the
// SAME_STEP autoreset inside its launch
static const int kOctetBatch = 16384;
// ... except the Servos kernels, which take the whole 512-entry register file (joint stops solved in registers): one
// wave per SIMD, 8192 envs
static const int kOctetBatchServos = 8192;

// What the choice depends on: the handle's settings and the call's.
struct StepFacts {
  int mode = MODE_RESET;
  int num_envs = 0;
  int lanes_per_env = 0;          // 0 = choose by batch size, 1 / 2 / 8 = forced (upkie_sim_set_lanes_per_env)
  bool spine = false;             // the spine observers run inside the step (upkie_sim_attach_observers)
  bool manifold = false;          // the Bullet-like contact model (upkie_sim_set_contact_manifold)
  bool ext_on_leg_links = false;  // a force buffer is set and one of its slots acts on a body other than the trunk
  bool randomized = false;        // inertial records or an external force buffer are set
  bool always_rand = false;       // UPKIE_ALWAYS_RAND_KERNELS=1 (the A/B of profiles/r05_ab_rand_instantiations.txt)
  bool default_scalars = false;   // the model's wheel / floor scalars are the default model's
  bool final_obs_set = false;     // upkie_sim_set_final_observation: the step calls complete a SAME_STEP autoreset themselves
  int autoreset_mode = UPKIE_AUTORESET_DISABLED;
  bool done_pass = false;         // the call is the DONE pass itself
  int packed = 0;
};

// lanes per env of the three kernel templates: step_kernel, step_kernel_pair (pair.hpp), step_kernel_octet (octet.hpp)
enum StepFamily { STEP_ONE_LANE = 1, STEP_PAIR = 2, STEP_OCTET = 8 };

// The instantiation: `family` and the template arguments behind MODE that the family has (the others stay as below).
struct StepInstance {
  int family = STEP_ONE_LANE;
  bool rand = false;             // every family: inertial records and external forces are read
  int waves = 1;                 // one lane: waves per SIMD the kernel is built for
  bool spine = false;            // one lane, pair: in-step spine observers (a separate instantiation: compiled in but
                                 // switched off they would still cost the common path 2 %)
  bool bullet = false;           // one lane, octet: Bullet-like contact model
  bool default_scalars = false;  // octet: the default model's scalars as constants
  bool in_place = false;         // octet: the SAME_STEP autoreset inside the launch (the second pass makes the whole
                                 // step a loop body: spills; hence its own instantiations)
  bool done_pass_follows = false;  // the other mappings: a second launch (the DONE pass) completes the SAME_STEP autoreset
  bool refused = false;            // no such kernel: MODE_PENDULUM_ROLLOUT on one lane
};

// Lanes per env of a step launch: eight (one quad per leg, one lane per body: octet.hpp) while that leaves the chip
// under-subscribed, two (one lane per leg: pair.hpp) up to one wave per SIMD, one beyond.
inline int step_lanes(const StepFacts& f) {
  // the eight-lane kernel restates neither the in-step spine observers nor forces on leg links, and addresses the state
  // with 32-bit byte offsets (state_words.hpp): a forced eight-lane mapping yields to the others beyond 2^32 bytes
  const bool eight_ok = !f.spine && (unsigned long long)f.num_envs * UPKIE_STATE_WORDS * sizeof(float) < (1ull << 32) && !f.ext_on_leg_links;
  // the Bullet-like contact model exists in the one- and eight-lane kernels (bullet_like.hpp, octet.hpp)
  const int fewer = f.manifold ? 1 : 2;
  int lanes;
  if (f.lanes_per_env == 8 || f.lanes_per_env == 2 || f.lanes_per_env == 1)
    lanes = (f.lanes_per_env == 8 && !eight_ok) || (f.lanes_per_env == 2 && f.manifold) ? fewer : f.lanes_per_env;
  else if (f.num_envs <= kOctetBatch && eight_ok)
    lanes = 8;
  else
    lanes = f.manifold || f.num_envs > kPairBatch ? 1 : 2;
  // the Servos kernels leave the eight-lane mapping earlier. (On the eight-lane Bullet-like kernel a joint within reach
  // of its stop is a row of the specification's own 50 sweeps, as on the one-lane kernels; what the mapping does not
  // restate is SEVERAL cached points on one tire, a robot lying flat on its side: upkie_sim_set_lanes_per_env(sim, 1)
  // selects the one-lane kernels)
  if (f.mode == MODE_SERVOS && lanes == 8 && f.lanes_per_env != 8 && f.num_envs > kOctetBatchServos) lanes = fewer;
  return lanes;
}

inline StepInstance select_step_instance(const StepFacts& f) {
  StepInstance k;
  k.family = step_lanes(f);
  // SAME_STEP autoreset completed by the step call itself (upkie_sim_set_final_observation): inside the launch on the
  // eight-lane mapping, by a second launch (the DONE pass) behind this one on the others
  const bool same_step = octet_resets_in_place(f.mode) && !f.done_pass && f.packed != 1 && f.final_obs_set &&
                         f.autoreset_mode == UPKIE_AUTORESET_DISABLED;
  k.done_pass_follows = same_step && k.family != STEP_OCTET;
  k.rand = f.randomized || (f.always_rand && k.family != STEP_OCTET);
  if (k.family == STEP_OCTET) {
    k.bullet = f.manifold;
    k.in_place = same_step;
    k.default_scalars = !f.manifold && f.default_scalars && octet_has_default_scalars(f.mode);
  } else if (k.family == STEP_PAIR) {
    k.spine = f.spine;
  } else if (f.mode == MODE_PENDULUM_ROLLOUT) {
    k.refused = true;  // several steps per launch need the two-lane mapping
  } else if (f.manifold) {
    k.bullet = true;
  } else {
    // more than two waves per SIMD in flight: favour occupancy over registers
    k.waves = f.num_envs >= kDenseBatch ? 2 : 1;
    k.spine = f.spine;
  }
  return k;
}

template <class Call>
static void with_flag(bool flag, Call&& call) {
  if (flag) call(std::true_type{});
  else call(std::false_type{});
}

// launch(family, rand, waves, spine, bullet, default_scalars, in_place), all std::integral_constant, for the
// instantiation `k` of mode MODE. The one list of what step_instances.hpp declares: an instance outside it reaches no launch.
template <int MODE, class Launch>
static void with_step_instance(const StepInstance& k, Launch&& launch) {
  using No = std::false_type;
  using OneWave = std::integral_constant<int, 1>;
  with_flag(k.rand, [&](auto rand) {
    if (k.family == STEP_OCTET) {
      const std::integral_constant<int, STEP_OCTET> octet{};
      with_flag(k.bullet, [&](auto bullet) {
        with_flag(k.default_scalars, [&](auto dflt) {
          with_flag(k.in_place, [&](auto in_place) {
            constexpr bool B = decltype(bullet)::value, D = decltype(dflt)::value, IP = decltype(in_place)::value;
            if constexpr ((!D || (octet_has_default_scalars(MODE) && !B)) && (!IP || octet_resets_in_place(MODE)))
              launch(octet, rand, OneWave{}, No{}, bullet, dflt, in_place);
          });
        });
      });
    } else if (k.family == STEP_PAIR) {
      with_flag(k.spine, [&](auto spine) { launch(std::integral_constant<int, STEP_PAIR>{}, rand, OneWave{}, spine, No{}, No{}, No{}); });
    } else if constexpr (MODE != MODE_PENDULUM_ROLLOUT) {
      const std::integral_constant<int, STEP_ONE_LANE> one_lane{};
      if (k.bullet) return launch(one_lane, rand, OneWave{}, No{}, std::true_type{}, No{}, No{});
      with_flag(k.spine, [&](auto spine) {
        if (k.waves == 2) launch(one_lane, rand, std::integral_constant<int, 2>{}, spine, No{}, No{}, No{});
        else launch(one_lane, rand, OneWave{}, spine, No{}, No{}, No{});
      });
    }
  });
}

}  // namespace upkie
