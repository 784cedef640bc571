/* klnmf_beta.h -- C-ABI of the beta-divergence cost on a context: the same loop on another cost function.
 *
 * An interface of its own beside klnmf.h (whose type, conventions and loop entry points it uses): int status returns,
 * klnmf_last_error(), every entry point naming the reference interface it stands in for.  The same library, libklnmf.so, exports
 * the symbols of every header.
 *
 * The cost.  With x = V + 1e-8 and y = W.H + 1e-8 in every term and optional weights Om >= 0 (klnmf_upload_weights):
 *     sum(Om o d_beta(x | y)),   d_2 = (x - y)^2 / 2,   d_0 = x/y - log(x/y) - 1,
 *     d_beta = (x^beta + (beta - 1) y^beta - beta x y^(beta-1)) / (beta (beta - 1))  otherwise;
 * beta = 1 is the context's own Kullback-Leibler loop and is no policy of this interface.
 * The rules.  A = Om o x o y^(beta-2), B = Om o y^(beta-1), gamma = 1/(2-beta) for beta < 1, 1 for 1 <= beta <= 2, 1/(beta-1) beyond:
 *     W <- W o ((A.H^T) / (B.H^T))^gamma        H <- H o ((W^T.A) / (W^T.B))^gamma        (a zero denominator: the factor 1)
 * One fit iteration of klnmf_run on a beta context: ratio pass on (W, H) -- the loss goes to the record and the stop rule
 * (nmf.py:214-220) --, W rule, a second ratio pass on (W_new, H), H rule, H's rows divided by 1e-16 + row sum and W's columns
 * multiplied by those sums (W.H is unchanged).  Every half step is a majorise-minimise step: the loss record does not rise.  A
 * transform (fit = 0) is the first ratio pass and the W rule.  Dense problems in KLNMF_PREC_F64 / KLNMF_PREC_F32 only.
 */
#ifndef KLNMF_BETA_H
#define KLNMF_BETA_H

#include "klnmf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cost function of the context's current problem: call after klnmf_set_problem (which returns a context to beta = 1) and the
 * uploads, before a loop.  beta != 1 takes the second n x f buffer B and, unless klnmf_upload_weights has taken them already, the
 * denominators' slabs and sums; beta = 1 hands them back and the context runs the KL loop again, bit for bit.
 * KLNMF_ERR_UNSUPP, the context as it was and usable: a CSR problem, a precision other than KLNMF_PREC_F64 / F32, a context with a
 * presence mask (klnmf_upload_presence), a member of a group or of a communicator or a context whose exchange buffers are a
 * caller's (klnmf_bind_exchange), and a loop that klnmf_loop_begin* opened and klnmf_loop_end has not closed (the cost may not change
 * between the pieces of a loop: there beta = 1 is refused too on a beta != 1 context; on a KL context it changes nothing and
 * returns KLNMF_OK).  A loop left open ends with its problem as well (klnmf_set_problem*, klnmf_release_problem) and with the next
 * klnmf_run; klnmf_group_run leaves none open on its members.  A klnmf_bind_exchange counts until the next klnmf_set_problem* or
 * the group's end, even one that binds the context's own buffers (klnmf_exchange_buffers) again.  KLNMF_ERR_ARG: a non-finite
 * beta, and in KLNMF_PREC_F32, where the kernels see beta rounded to fp32, a beta that rounds to 1 or to 0 without being it (the
 * general cost divides by beta (beta - 1)).  On a beta != 1 context the
 * sharded, group and communicator loops refuse where they refuse a weighted one, klnmf_bind_exchange refuses, and so do klnmf_error
 * and klnmf_step_Q / _W / _H, which are the KL cost's: klnmf_beta_loss and klnmf_beta_step stand in their place.
 * Stands in for nmf.py:293 ("Helpers for beta divergence and related updates", followed by nothing):
 * the reference has no counterpart. */
int klnmf_set_divergence(klnmf_ctx *ctx, double beta);
/* The beta of the current problem (1 without klnmf_set_divergence).  nmf.py:293: the reference has no counterpart. */
int klnmf_get_divergence(klnmf_ctx *ctx, double *beta);
/* The beta cost of the context's current V, W, H and weights (beta = 1: klnmf_error's value).  Stands in for the `error` of
 * nmf.py:297-310 under the cost of nmf.py:293: the reference has no counterpart. */
int klnmf_beta_loss(klnmf_ctx *ctx, double *loss);
/* One rule from a freshly formed A and B at the current (W, H).  which = 0: the W rule (nmf.py:338-343 under the beta cost);
 * which = 1: the H rule with the normalisation of H's rows and its compensation on W's columns (nmf.py:349-350 under the beta
 * cost).  KLNMF_ERR_UNSUPP on a beta = 1 context (klnmf_step_Q / _W / _H are its steps), KLNMF_ERR_ARG for another `which`.
 * nmf.py:293: the reference has no counterpart. */
int klnmf_beta_step(klnmf_ctx *ctx, int which);

#ifdef __cplusplus
}
#endif
#endif /* KLNMF_BETA_H */
