// fleet_c.hpp — the object behind a sortham_fleet handle (shared by fleet_c.cpp and tick_loop.cpp;
// include/smpc_host.h is the interface).
#ifndef SORTHAM_HOST_FLEET_C_HPP_
#define SORTHAM_HOST_FLEET_C_HPP_

#include <memory>
#include <string>
#include <vector>

#include "fleet.hpp"
#include "optimizer_c.hpp"

struct sortham_fleet
{
  std::unique_ptr<sortham_ns::FleetOptimizer> fleet;
  // the members' handles, for their last_error; one is only touched while fleet->member(i) says
  // the object still exists
  std::vector<sortham_optimizer *> handles;
  // one round's arguments, kept between rounds (the plans keep their capacity)
  std::vector<sortham_ns::Pose2D> poses, goals;
  std::vector<sortham_ns::Twist2D> speeds;
  std::vector<sortham_ns::models::Path> plans;
  std::vector<float> tolerances;
  std::vector<uint8_t> take;
  std::vector<sortham_ns::MemberResult> results;
  std::string err;
};

#endif
