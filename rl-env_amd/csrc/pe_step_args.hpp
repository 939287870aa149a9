// pe_step_args.hpp -- StepArgs, the one argument struct of every env kernel, and the sizes all
// of them share: kBlock (envs per workgroup of the lane-per-env kernels) and kTabFloats (the
// Tables image at the head of every kernel's LDS; its map is in pe_device.hpp).
// (a fragment of plantos_batch.hip's anonymous namespace; include after pe_device.hpp and pe_coop.hpp)
#pragma once

constexpr int kBlock = 64;      // envs per workgroup (one wave)
constexpr int kTabFloats = (int)(sizeof(Tables) / sizeof(float));  // whole Tables struct in LDS
static_assert(sizeof(Tables) % 16 == 0, "LDS regions after the tables stay 16-B aligned");

struct StepArgs {
  State st;
  Geo g;
  Rules rl;
  int n;
  int autoreset;
  int act_bytes;
  int coop_max_done;  // step kernel: wave-cooperative resets up to this many done envs per block
  const void* actions;
  float* obs;
  uint8_t* obs_codes;   // byte-coded tile kernels: the obs as codes (pe_step_codes) instead of obs
  float* reward;
  uint8_t* term;
  uint8_t* trunc;
  float* tobs;
  double* ep_ret_out;
  int32_t* ep_len_out;
  int32_t* tinfo;       // terminal _get_info rows of done envs (may be NULL)
  Prefetch pf;          // prefetched resets (pe_coop.hpp); pf.scal == NULL: off
  int stagger;          // sector kernel: start delay per block quarter, units of 512 cycles
  const uint8_t* mask;  // reset kernel
};
