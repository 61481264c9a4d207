// Test-only: the oracle's mock of the device ABI (oracle/mock_hip.cpp: an implementation of include/lasso_hip.h alone) as ONE translation unit with any set of the optional
// entry points on top, each a fragment selected by -DMOCK_EXT_<NAME> (tests/mockbuild.py, which also knows what a fragment requires).  A fragment holds its own entry points
// and helpers and includes no other .cpp; "device" pointers are host pointers here.  Linked with lasso_amd/host/prover_capi.cpp, whose weak references to the selected
// entries then resolve — so the host takes its device routes on the CPU — while every other optional entry stays absent.
#ifdef MOCK_EXT_CUSTOM   // custom wraps the mock's two entry points that take a strategy: they are compiled under other names, and the fragment defines the ABI's
#define lasso_sumcheck_combine_round mock_builtin_combine_round
#define lasso_combine_claim mock_builtin_combine_claim
#endif
#include "../../oracle/mock_hip.cpp"
#ifdef MOCK_EXT_CUSTOM
#undef lasso_sumcheck_combine_round
#undef lasso_combine_claim
#include "mock_custom_wrap.cpp"
#endif
#ifdef MOCK_EXT_WIRE
#include "mock_wire_wrap.cpp"
#endif
#ifdef MOCK_EXT_MSM_POINTS
#include "mock_msm_points_wrap.cpp"
#endif
#ifdef MOCK_EXT_OPERANDS
#include "mock_operands_wrap.cpp"
#endif
#ifdef MOCK_EXT_GENS
#include "mock_gens_wrap.cpp"
#endif
#ifdef MOCK_EXT_MLE
#include "mock_mle_wrap.cpp"
#endif
#ifdef MOCK_EXT_VALUES
#include "mock_values_wrap.cpp"
#endif
#ifdef MOCK_EXT_POLY
#include "mock_poly_wrap.cpp"
#endif
