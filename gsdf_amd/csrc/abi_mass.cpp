// abi_mass.cpp -- C ABI (include/gsdf_hip.h, "indexed meshes: mass properties"): the entry point that runs on the host alone,
// gsdf_hip_inertia_principal (the arithmetic: mass_host.h). Plain C++ without a HIP header: with a `fail` of its own a stand-alone
// program links this file as it is (tests/test_mass_ref.py runs one under AddressSanitizer and UBSan).
#include <string>

#include "mass_host.h"

int fail(int code, const std::string& msg);  // abi_host.cpp: sets the calling thread's gsdf_hip_last_error text, returns code

extern "C" int gsdf_hip_inertia_principal(const double inertia[6], double moments[3], double axes[9]) {
  if (!inertia || !moments || !axes) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!mass::principal(inertia, moments, axes)) return fail(GSDF_ERR_BAD_ARGUMENT, "inertia principal: a NaN or infinite entry");
  return GSDF_OK;
}
