// optimizer_c.hpp — what the C faces of the host classes share (not installed: include/smpc_host.h
// is the interface): the object behind a sortham_optimizer handle.
#ifndef SORTHAM_HOST_OPTIMIZER_C_HPP_
#define SORTHAM_HOST_OPTIMIZER_C_HPP_

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/smpc_host.h"
#include "optimizer.hpp"

namespace sortham_ns = SORTHAM_HOST_NS;

namespace sortham_c_detail
{
// the class plus the one call the C face adds: a footprint handed over on its own, not with a costmap
struct OptimizerWithFootprint : sortham_ns::Optimizer
{
  void applyFootprint(const std::vector<double> & xy, double radius, double layer_scale)
  {
    if (!ctx_ || xy.empty()) {return;}
    if (smpc_set_footprint(ctx_, xy.data(), static_cast<uint32_t>(xy.size() / 2), radius, layer_scale) != SMPC_OK) {
      throw std::runtime_error(std::string("smpc_set_footprint: ") + smpc_last_error(ctx_));
    }
  }
};
}  // namespace sortham_c_detail

struct sortham_optimizer
{
  sortham_c_detail::OptimizerWithFootprint opt;
  std::string err;
  // sortham_optimizer_set_footprint: kept for the contexts initialize() builds later
  std::vector<double> footprint_xy;
  double circumscribed_radius{0};
  double layer_cost_scaling_factor{-1.0};
};

#endif
