// mlp_instances.hpp -- which instantiation of a kernel template <int W, int ACT> runs an UpkieMlpShape: shared by the
// translation units that launch such kernels (trainer_abi.hip: policy and time-limit bootstrap; ppo_abi.hip: gradient).
#pragma once

#include <type_traits>

#include "policy_mlp.hpp"

// The instantiation of a kernel template <int W, int ACT> that runs `shape`: launch(width class, activation), both as
// std::integral_constant. The one list of the width classes and activations that have kernels.
template <class Launch>
static auto for_mlp_instance(const UpkieMlpShape& shape, Launch&& launch) {
  auto with_width = [&](auto width) {
    if (shape.activation == UPKIE_MLP_TANH) return launch(width, std::integral_constant<int, UPKIE_MLP_TANH>{});
    return launch(width, std::integral_constant<int, UPKIE_MLP_RELU>{});
  };
  switch (upkie::mlp_width_class(shape)) {
    case 16: return with_width(std::integral_constant<int, 16>{});
    case 32: return with_width(std::integral_constant<int, 32>{});
    case 64: return with_width(std::integral_constant<int, 64>{});
    case 128: return with_width(std::integral_constant<int, 128>{});
    default: return with_width(std::integral_constant<int, 256>{});
  }
}
