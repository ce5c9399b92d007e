// Tag types of the hand-scheduled loops (gemm_bf16.hip, gemm_fp8.hip, attn_fwd.hip): a loop body written once as a generic lambda takes its buffer / phase
// index as one of these, so the index is a compile-time constant inside the body (register arrays stay registers) while the call sites read as a schedule.
#pragma once
#include <type_traits>

namespace rga3 {

// which half-tile of a K step a stage call loads: rows 0 / 1 of A, columns 0 / 1 of B
using K_A0 = std::integral_constant<int, 0>;
using K_A1 = std::integral_constant<int, 1>;
using K_B0 = std::integral_constant<int, 2>;
using K_B1 = std::integral_constant<int, 3>;
// operand half or buffer (H), slot of the attention K / V ring (S), third of the 3-row-block form (U), and a compile-time flag
using H0 = std::integral_constant<int, 0>;
using H1 = std::integral_constant<int, 1>;
using S0 = std::integral_constant<int, 0>;
using S1 = std::integral_constant<int, 1>;
using U0 = std::integral_constant<int, 0>;
using U1 = std::integral_constant<int, 1>;
using U2 = std::integral_constant<int, 2>;
using TRUE_T = std::true_type;
using FALSE_T = std::false_type;

}  // namespace rga3
