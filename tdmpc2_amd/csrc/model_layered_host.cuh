// Layered family: the stages of tdmpc2_plan_model_rollout / model_losses (the forward half of TDMPC2._update,
// tdmpc2/tdmpc2.py:268-283) on lay_gemm / lay_hidden / lay_dynamics.  model_route.h decides which stages run:
//   MS_DYN    per step: the recorded actions into X's action columns, the dynamics chain over the B rows (in place, as in planning),
//             then the new latent out of X into zs[t + 1] (l_model_get_z).
//   MS_HEADS  X <- [zs[:-1] | actions] for all H * B flattened rows at once; per chain (reward, every Q head) the two hidden
//             layers, the head GEMM and l_model_head_rows -- every GEMM sees H * B rows, not B.
//   MS_TERM   the same on (H + 1) * B rows of zs with the termination head, in pieces of the workspace's rows.
// Everything runs on the caller's stream.  Included by k_layered.hip inside namespace tdk, after layered_host.cuh.
#pragma once

namespace {
int model_init_rows(tdmpc2_plan *h, hipStream_t st, const float *z, size_t rows, size_t rows_p) {
    const Layered &L = h->lay;
    if (h->split) hipLaunchKernelGGL(l_init_rows_s, dim3((unsigned)(rows_p / 32)), dim3(256), 0, st, L.X, L.Kin, h->cfg.latent_dim, z, (int)rows);
    else hipLaunchKernelGGL(l_init_rows, dim3((unsigned)rows_p), dim3(256), 0, st, L.X, L.Kin, h->cfg.latent_dim, z, (int)rows);
    LAUNCH_CHECK();
    return 0;
}
// X[row, L + a] <- actions[t, row, a] for `rows` rows of a [steps, rows, A] tensor
int model_set_actions(tdmpc2_plan *h, hipStream_t st, const float *actions, int steps, int t, size_t rows) {
    const Layered &L = h->lay;
    const int A = h->cfg.action_dim;
    if (h->split)
        hipLaunchKernelGGL(l_set_action_s, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, st, L.X, L.Kin, h->cfg.latent_dim, A, (int)rows, steps, t,
                           (int)rows, actions, (int)rows, 0);
    else
        hipLaunchKernelGGL(l_set_action, dim3((unsigned)((rows * A + 255) / 256)), dim3(256), 0, st, L.X, L.Kin, h->cfg.latent_dim, A, (int)rows, steps, t,
                           (int)rows, actions, (int)rows, 0);
    LAUNCH_CHECK();
    return 0;
}
// hidden layers + head GEMM of one chain over the rows in X, then the row kernel
int model_chain(tdmpc2_plan *h, hipStream_t st, const HostNet &net, int slot, size_t rows, size_t rows_p, ModelHeadRowsParams hp) {
    const Layered &L = h->lay;
    int rc;
    if ((rc = lay_hidden(h, st, net, slot, rows, rows_p, (int)rows_p, nullptr, false))) return rc;
    if ((rc = lay_gemm(h, st, L.HB, L.Mp, rows_p, (int)rows_p, net.l[2], 0, 0, -1, nullptr, L.LG, L.ldl))) return rc;
    hp.lg = L.LG; hp.ld = L.ldl; hp.rows = (int)rows;
    hipLaunchKernelGGL(l_model_head_rows, dim3((unsigned)((rows + RW_THREADS / 64 - 1) / (RW_THREADS / 64))), dim3(RW_THREADS), 0, st, hp);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

int lay_model(tdmpc2_plan *h, hipStream_t st, const ModelRoute &r, int B, int H, const float *actions, float *zs, bool target,
              const int *row_task, const ModelOutArgs &out, const ModelLossArgs &ls) {
    const tdmpc2_plan_cfg &c = h->cfg;
    Layered &L = h->lay;
    const int Ld = c.latent_dim;
    struct Restore {  // the helpers read these from the handle (as in lay_value)
        Layered &L; const HostNet *q; const float *bt; const int *re;
        ~Restore() { L.qarr = q; L.bias_tab = bt; L.row_env = re; }
    } restore{L, L.qarr, L.bias_tab, L.row_env};
    L.qarr = target ? h->tq : h->q;
    if (c.multitask) { L.bias_tab = h->beff_tab; L.row_env = row_task; }
    const unsigned int *err = (h->split && L.fuse_ln) ? h->cl_err_dev : nullptr;
    int rc;
    if ((rc = lay_arrive_reset(h, st))) return rc;
    if (r.st[MS_DYN].run) {
        const size_t rows = (size_t)B, rows_p = round_up(rows, GBM);
        if ((rc = model_init_rows(h, st, zs, rows, rows_p))) return rc;
        for (int t = 0; t < r.st[MS_DYN].steps; ++t) {
            if ((rc = model_set_actions(h, st, actions, H, t, rows))) return rc;
            if ((rc = lay_dynamics(h, st, rows, rows_p, (int)rows_p))) return rc;
            ModelGetZParams g{L.X, L.Kin, Ld, B, h->split ? 1 : 0, zs + (size_t)(t + 1) * B * Ld, err};
            hipLaunchKernelGGL(l_model_get_z, dim3((unsigned)((rows * Ld + 255) / 256)), dim3(256), 0, st, g);
            LAUNCH_CHECK();
        }
    }
    if (r.st[MS_HEADS].run) {
        const size_t rows = (size_t)H * B, rows_p = round_up(rows, GBM);
        if ((rc = model_init_rows(h, st, zs, rows, rows_p))) return rc;
        if ((rc = model_set_actions(h, st, actions, 1, 0, rows))) return rc;
        const int nbc = c.num_bins > 1 ? c.num_bins : 1;
        for (int k = 0; k < r.nchain; ++k) {
            ModelHeadRowsParams hp{};
            hp.B = B; hp.row0 = 0; hp.ls = ls; hp.ls.err = err;
            if (r.chain[k] == MC_REWARD) {
                hp.kind = MK_REW; hp.logits_out = out.rew_logits; hp.val_out = out.rew;
                if ((rc = model_chain(h, st, h->rew, BE_REW, rows, rows_p, hp))) return rc;
            } else {
                const int i = r.chain[k] - MC_Q0;
                hp.kind = MK_Q0 + i;
                hp.logits_out = out.q_logits ? out.q_logits + (size_t)i * rows * nbc : nullptr;
                hp.val_out = out.q ? out.q + (size_t)i * rows : nullptr;
                if ((rc = model_chain(h, st, L.qarr[i], BE_Q0 + i, rows, rows_p, hp))) return rc;
            }
        }
    }
    if (r.st[MS_TERM].run) {
        const size_t total = (size_t)(H + 1) * B, piece = (size_t)r.st[MS_TERM].rows;
        for (size_t off = 0; off < total; off += piece) {
            const size_t rows = std::min(piece, total - off), rows_p = round_up(rows, GBM);
            if ((rc = model_init_rows(h, st, zs + off * Ld, rows, rows_p))) return rc;
            ModelHeadRowsParams hp{};
            hp.B = B; hp.row0 = (long)off; hp.ls = ls; hp.ls.err = err; hp.kind = MK_TERM; hp.val_out = out.term_logit;
            if ((rc = model_chain(h, st, h->term, -1, rows, rows_p, hp))) return rc;
        }
    }
    return 0;
}
