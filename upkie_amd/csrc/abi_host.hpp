// abi_host.hpp -- what the translation units of the C-ABI (upkie_hip.hip: simulator, MPC, observers; trainer_abi.hip:
// policy, normalisation, episodes, rollout; ppo_abi.hip: the PPO update) share on the host: the per-thread error message
// and the one-line error exits.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/upkie_hip.h"

// The message of the calling thread's last failed call that had no handle to keep it: ONE object for the whole library
// (defined in upkie_hip.hip), what the three *_last_error(NULL) return.
extern thread_local std::string g_create_error;

static inline int fail(int status, const std::string& msg) {
  g_create_error = msg;
  return status;
}

// UPKIE_ERR_NO_DEVICE (and the message set) when no HIP device is visible, else UPKIE_OK. Asked after every argument
// check, so that a wrong argument is reported as such on a machine without a GPU too.
static inline int no_device() { return upkie_hip_device_count() > 0 ? UPKIE_OK : fail(UPKIE_ERR_NO_DEVICE, "no HIP device visible"); }

// The status of the launches a handle-free entry point has just made (or of `err`, when a call before them failed).
static inline int launch_status(hipError_t err = hipGetLastError()) {
  return err == hipSuccess ? UPKIE_OK : fail(UPKIE_ERR_HIP, hipGetErrorString(err));
}
