// Lanczos estimate of lambda_min(H + J' Sigma J) on a KKT handle (lanczos.hip): okkt_kkt_min_eig and the
// certificate that okkt_kkt_ipopt_strategy_eig skips attempts with.
#pragma once
#include "kkt_state.h"

namespace okkt {

// okkt_kkt_min_eig behind its argument checks of the handle (k is not NULL): everything else is checked here
int kk_min_eig(okkt_kkt_s* k, int32_t max_steps, double tol, int32_t scaled, okkt_kkt_eig_info* info, double* v_out);
// the workspace of the estimate (allocated on the first call, grown for a larger max_steps): released with the handle
void lanczos_release(okkt_kkt_s* k);

}  // namespace okkt
