// libklnmf.so, the beta-divergence unit: the entry points of include/klnmf_beta.h -- the cost function of a context's problem
// (klnmf_set_divergence: buffers and refusals), its loss and its single steps.  The loop itself is klnmf_run's: the pieces of an
// iteration branch on c->beta_on() in api_loop.hip beside c->weighted(), on the kernels and policies of beta.hip.h.  Every entry
// stands in for nmf.py:293 ("Helpers for beta divergence and related updates", followed by nothing): the reference has no
// counterpart.
#include "ctx.hip.h"
#include "../../include/klnmf_beta.h"

namespace klnmf_host {
namespace {

void beta_drop(klnmf_ctx *c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    c->dfree(c->Bt);      // (hpart stays the problem's: k doubles where klnmf_set_divergence took it)
    if (!c->weighted()) { c->dfree(c->Dpart); c->dfree(c->denom); c->dfree(c->WDpart); }
    c->beta = 1.0;
}

}  // namespace
}  // namespace klnmf_host

extern "C" {

int klnmf_set_divergence(klnmf_ctx *c, double beta) {
    return guarded([&] {
        need_problem(c);
        const std::string who = "klnmf_set_divergence";
        if (!std::isfinite(beta)) fail(KLNMF_ERR_ARG, who + ": beta must be finite");
        if (beta == 1.0) {      // the KL loop again: nothing of the beta cost stays
            if (c->beta_on() && c->pieces_open) fail(KLNMF_ERR_UNSUPP, who + ": a loop is open on this context; klnmf_loop_end first");
            if (c->beta_on()) beta_drop(c);
            return;
        }
        if (c->sparse) fail(KLNMF_ERR_UNSUPP, who + ": CSR problems have no beta kernels (the ratio lives on the stored entries only)");
        if (c->prec != KLNMF_PREC_F64 && c->prec != KLNMF_PREC_F32)
            fail(KLNMF_ERR_UNSUPP, who + ": the beta kernels exist in KLNMF_PREC_F64 and KLNMF_PREC_F32 only");
        if (c->prec == KLNMF_PREC_F32 && beta != 0.0 && ((float)beta == 1.0f || (float)beta == 0.0f))
            fail(KLNMF_ERR_ARG, who + ": in KLNMF_PREC_F32 the kernels see beta rounded to fp32, and this beta rounds to 1 or to 0 "
                                      "without being it (the general cost divides by beta (beta - 1)); give 1 or 0 itself");
        if (c->presence())
            fail(KLNMF_ERR_UNSUPP, who + ": the problem holds a presence mask (klnmf_upload_presence), and the beta rules have no masked "
                                         "form; klnmf_clear_weights first and upload the mask as weights");
        if (c->pieces_open)
            fail(KLNMF_ERR_UNSUPP, who + ": a loop is open on this context (klnmf_loop_begin; over row shards its exchange carries no "
                                         "denominator of the beta H rule) and the cost may not change between its pieces; klnmf_loop_end first");
        if (c->comm != nullptr || c->exchange_bound)
            fail(KLNMF_ERR_UNSUPP, who + ": the context is a member of a group or of a communicator, or its exchange buffers are bound to a "
                                         "caller's (klnmf_bind_exchange), and that exchange carries no denominator of the beta H rule");
        if (c->beta_on()) { c->beta = beta; return; }      // (the buffers are there)
        HIPCHK(hipStreamSynchronize(c->stream));
        const size_t es = c->esize(), n = (size_t)c->n, f = (size_t)c->f, k = (size_t)c->k;
        const bool have_den = c->weighted();                // (klnmf_upload_weights took the denominators' slabs and sums)
        const bool have_sums = c->hpart != nullptr;         // (long rows: the problem holds [k][hseg_n] already)
        void *bt = nullptr, *sums = nullptr;
        try {
            bt = c->dalloc(n * f * es);
            if (!have_sums) sums = c->dalloc(sizeof(double) * k);
            if (!have_den) {
                c->Dpart = c->dalloc((size_t)c->nsplit * k * f * es);
                c->denom = c->dalloc(k * f * es);
                if (c->wsplit > 1) c->WDpart = c->dalloc((size_t)c->wsplit * n * k * es);
            }
        } catch (...) {                                     // all or nothing: a failed call leaves the problem at beta = 1
            (void)hipStreamSynchronize(c->stream);
            if (!have_den) { c->dfree(c->Dpart); c->dfree(c->denom); c->dfree(c->WDpart); }
            c->dfree(bt); c->dfree(sums);
            throw;
        }
        c->Bt = bt;
        if (!have_sums) c->hpart = (double *)sums;
        c->beta = beta;
    });
}

int klnmf_get_divergence(klnmf_ctx *c, double *beta) {
    return guarded([&] {
        need_problem(c);
        if (!beta) fail(KLNMF_ERR_ARG, "klnmf_get_divergence: null destination");
        *beta = c->beta;
    });
}

int klnmf_beta_loss(klnmf_ctx *c, double *loss) {
    if (c && c->have_problem && !c->beta_on()) return klnmf_error(c, loss);      // beta = 1: the KL loss, by its own code
    return guarded([&] {
        need_problem(c);
        reset_state(c);
        beta_ratio(c, c->cur, true);
        double h[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h, c->loss_xchg, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (loss) *loss = h[0];
    });
}

int klnmf_beta_step(klnmf_ctx *c, int which) {
    return guarded([&] {
        need_problem(c);
        if (!c->beta_on()) fail(KLNMF_ERR_UNSUPP, "klnmf_beta_step: the context runs the KL loop (beta = 1); its steps are klnmf_step_Q / _W / _H");
        if (which != 0 && which != 1) fail(KLNMF_ERR_ARG, "klnmf_beta_step: which must be 0 (the W rule) or 1 (the H rule)");
        reset_state(c);
        beta_ratio(c, c->cur, false);
        if (which == 0) {
            beta_rule_W(c);
            c->cur ^= 1;
        } else {
            beta_rule_H(c, c->cur, false);
        }
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

}  // extern "C"
