/* cassie_trpo.h -- fused policy kernels of the TRPO outer loop: the counterpart of what rllab's TRPO
 * (rllab/envs/trpo_cassie.py:21-42: GaussianMLPPolicy 32x32 tanh, conjugate-gradient optimiser with Fisher-vector products by
 * double backprop through the mean KL) evaluates on the sampled batch, for the batch sizes the vectorised environment produces
 * (65 536 envs x 8 steps = 524 288 samples per rank and iteration).
 *
 * The policy is mean(obs) = W3 tanh(W2 tanh(W1 obs + b1) + b2) + b3 with a state-independent log-std; float32, row-major weights
 * as torch.nn.Linear stores them (W1 [32][obs_dim], W2 [32][32], W3 [act_dim][32]).  Plain device pointers and sizes; every call
 * enqueues on `stream` (a hipStream_t, 0 = default) and returns 0 or a negative CASSIE_E* code (cassie_vec.h).
 *
 * Both entry points write PARTIAL sums, one row per wavefront of the launch: partial [n_rows][CassieTrpoParamCount] float32 with the
 * row layout [gW1 | gb1 | gW2 | gb2 | gW3 | gb3]; the caller adds the rows up (one reduction) -- and all-reduces the result over
 * ranks, exactly where the unfused version did.  CassieTrpoPartialRows() says how many rows a launch over n samples writes.
 */
#ifndef CASSIE_TRPO_H_
#define CASSIE_TRPO_H_

#ifdef __cplusplus
extern "C" {
#endif

/* parameters of the mean network: 32 * obs_dim + 32 + 32 * 32 + 32 + act_dim * 32 + act_dim; 0 for an unsupported shape
 * (supported: obs_dim 26 or 17, act_dim 6 or 7) */
int CassieTrpoParamCount(int obs_dim, int act_dim);
int CassieTrpoPartialRows(int n_samples);

/* Fisher-vector product of the mean network, (1/n) J' S J v: J = d mean / d theta at the CURRENT weights (forward mode per sample
 * along the direction dW1..db3, activations recomputed), S = diag(prec[act_dim]) the precision of the old Gaussian, then reverse
 * mode back to the parameters.  scale is the 1/n (n of the whole job) the caller wants folded in. */
int CassieTrpoFvp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* W3, const float* b3, const float* dW1, const float* db1, const float* dW2, const float* db2, const float* dW3,
                  const float* db3, const float* prec, float scale, float* partial_dev, void* stream);

/* Vector-Jacobian product J' w for per-sample cotangents w [n][act_dim] on the mean (the policy gradient of the surrogate loss:
 * w = d loss / d mean, evaluated by the caller). */
int CassieTrpoVjp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* W3, const float* b3, const float* w_dev, float* partial_dev, void* stream);

/* Line search of the TRPO step on the sampled batch (what rllab's f_loss / f_constraint evaluate per backtrack): for the mean network
 * AT THE GIVEN WEIGHTS and log-std log_std_new [act_dim], against the old Gaussian (old_mean [n][act_dim], log_std_old [act_dim]):
 *   partial[row][0] = sum_s -exp(ll_new(act_s) - ll_old(act_s)) adv_s,   partial[row][1] = sum_s KL(old_s || new_s)
 * (GaussianMLPPolicy.log_likelihood / .kl of cassierl_amd/trpo.py), float64, one row per wavefront (CassieTrpoPartialRows); the
 * caller adds the rows and divides by the job's n. */
int CassieTrpoSurrogate(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* W3, const float* b3, const float* log_std_new, const float* log_std_old, const float* act_dev,
                        const float* adv_dev, const float* old_mean_dev, double* partial_dev, void* stream);

/* The vector work of one conjugate-gradient iteration (rllab/misc/krylov.py: cg) between two Fisher-vector products, one launch: with the
 * parameter vector laid out as [.. | log_std block at ls_off, n_ls entries | ..] and Ap_mean [n - n_ls] = the mean network's part of F p
 * (rows of CassieTrpoFvp added up, summed over ranks, in the order of the remaining entries):
 *   Ap = Ap_mean (+ hls o p on the log_std block) + reg p;  alpha = rr / p.Ap;  x += alpha p;  r -= alpha Ap;  rr' = r.r;
 *   p = r + (rr' / rr) p;  scal = {rr', running}: once rr' < tol the step length stays 0 (cg's early exit without a host read-back). */
int CassieTrpoCgUpdate(int n, int ls_off, int n_ls, const float* Ap_mean_dev, const float* hls_dev, float reg, float tol, float* x_dev, float* r_dev, float* p_dev,
                       float* scal_dev, void* stream);

/* One policy step of the sampler for n environments in ONE launch (the counterpart of GaussianMLPPolicy.get_actions + rllab's
 * normalize() wrapper, rllab/envs/trpo_cassie.py:13,21-27): obs float64 [n][obs_dim] as the environment wrote it ->
 *   obs32 [n][obs_dim] (the policy's float32 view, kept for the update), mean [n][act_dim] = mean network, act [n][act_dim] = mean +
 *   noise * exp(log_std) (noise: standard normal numbers of the caller, row stride act_dim), and
 *   env_actions float64 [n][act_dim] = clip(low + (act + 1) / 2 * (high - low), low, high): what CassieVecStep consumes. */
int CassieTrpoPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2,
                         const float* b2, const float* W3, const float* b3, const float* log_std, const float* noise_dev,
                         const double* low_dev, const double* high_dev, float* obs32_dev, float* mean_dev, float* act_dev,
                         double* env_actions_dev, void* stream);

/* Sampler bookkeeping of one Env.step for n environments in one launch (the per-path clocks and returns rllab's sampler keeps on the
 * host; cassierl_amd/trpo.py: collect): with rew / done as CassieVecStep wrote them,
 *   rew_row[i] = rew[i], t_row[i] = path_t[i]  (this step's rows of the batch),  path_ret[i] += rew[i], path_t[i] += 1,
 *   cut = done[i] || path_t[i] >= max_path_length  (rllab truncates paths there),  cut_row[i] = cut (one byte, 0 / 1),
 *   a cut path adds (1, path_ret[i]) to its workgroup's row of partial [CassieTrpoSamplerRows(n)][2] and restarts: path_ret[i] = path_t[i] = 0.
 * The rows are summed in a fixed order inside the kernel; the caller adds them up. */
int CassieTrpoSamplerRows(int n_envs);
int CassieTrpoSamplerStep(const double* rew_dev, const unsigned char* done_dev, int n, long long max_path_length, long long* path_t_dev, double* path_ret_dev,
                          double* rew_row_dev, long long* t_row_dev, unsigned char* cut_row_dev, double* partial_dev, void* stream);

/* ---- the baseline side: rllab's LinearFeatureBaseline (trpo_cassie.py:30) on the [T][n] batch of the vectorised environment.
 * Features of a sample: [o, o^2, a, a^2, a^3, 1] with o = clip(obs, -10, 10) [obs_dim] and a = path clock / 100, evaluated in float32 as the
 * torch expressions of cassierl_amd/trpo.py evaluate them, used in float64; CassieTrpoBaselineFeatures(obs_dim) = 2 obs_dim + 4 (0: unsupported). */
int CassieTrpoBaselineFeatures(int obs_dim);

/* values[s] = features(obs[s], t[s]) . coeffs  (obs float32 [m][obs_dim], t int64 [m], coeffs float64 [features]) */
int CassieTrpoBaselinePredict(const float* obs_dev, const long long* t_dev, int m, int obs_dim, const double* coeffs_dev, double* out_dev, void* stream);

/* One lane per environment, backwards over the T steps of its column of the batch (sample s = step * n + env):
 *   value = features . coeffs (0 with coeffs = NULL: the first iteration),
 *   returns[s] = rew[s] + gamma * returns[next step] * !cut[s]  (bootstrapped behind the last step with last_value [n], NULL = 0),
 *   adv[s] = returns[s] - value  (gae_lambda = 1),
 * and partial[(n + 255) / 256][2] = per workgroup (sum adv, sum adv^2), fixed order: what the advantage normalisation needs. */
int CassieTrpoReturnsAdvantages(const float* obs_dev, const long long* t_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, int obs_dim,
                                const double* coeffs_dev, const double* last_value_dev, double gamma, double* returns_dev, double* adv_dev, double* partial_dev,
                                void* stream);

/* Normal equations of the baseline's ridge regression: Z'Z for Z = [features | y] (m samples, 2 obs_dim + 5 columns padded to a multiple
 * of 16) on the FP64 matrix cores.  partial [CassieTrpoGramRows()][CassieTrpoGramRowSize(obs_dim)]: per wavefront the UPPER 16 x 16 blocks
 * (r <= c, r-major) of the Gram matrix, each row-major; the caller adds the rows up: X'X = Z'Z[:features, :features], X'y = Z'Z[:features, features]. */
/* (A + reg I) x = b, A [F][F] symmetric positive semi-definite (F = CassieTrpoBaselineFeatures(obs_dim): 56, 38 or -- obs_dim 45 -- 94), by Cholesky on the device; a failed factorisation or a non-finite
 * solution retries with ten times the regulariser, five times in all (LinearFeatureBaseline.fit's rule, without a host read-back). */
int CassieTrpoRidgeSolve(const double* A_dev, const double* b_dev, int F, double reg, double* x_dev, void* stream);
int CassieTrpoGramRows(void);
int CassieTrpoGramRowSize(int obs_dim);
int CassieTrpoBaselineGram(const float* obs_dev, const long long* t_dev, const double* y_dev, int m, int obs_dim, double* partial_dev, void* stream);

/* ---- width-128 policy: the GaussianMLPPolicy((128, 128)) of rllab/envs/vpg_cassie.py (cassierl_amd/vpg.py).  The mean network is the one
 * above with 128 hidden units per layer (W1 [128][obs_dim], W2 [128][128], W3 [act_dim][128]); b1, W2, b2 and W3 must be 16-byte aligned
 * (CASSIE_EINVAL otherwise).  Same row layout and conventions as the width-32 entry points. */

/* 128 * obs_dim + 128 + 128 * 128 + 128 + act_dim * 128 + act_dim; 0 for an unsupported shape (obs_dim 26 or 17, act_dim 6 or 7) */
int CassiePgParamCount(int obs_dim, int act_dim);

/* CassieTrpoPolicyStep for the 128-128 network (obs_dim 26, act_dim 6 or 7), one launch */
int CassiePgPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* W3, const float* b3, const float* log_std, const float* noise_dev,
                       const double* low_dev, const double* high_dev, float* obs32_dev, float* mean_dev, float* act_dev,
                       double* env_actions_dev, void* stream);

/* J' w of the 128-128 mean network for cotangents w [n][act_dim]: partial [CassiePgPartialRows(n)][CassiePgParamCount] float32, rows
 * [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], one per workgroup; the caller adds the rows (fixed order inside each row: a run repeats bit for bit). */
int CassiePgPartialRows(int n_samples);
int CassiePgVjp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* W3, const float* b3, const float* w_dev, float* partial_dev, void* stream);

/* Lasagne's Adam step (lasagne.updates.adam) in place on n float32 parameters, one launch; t = the step count after its increment (>= 1):
 *   a = lr sqrt(1 - beta2^t) / (1 - beta1^t);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  theta -= a m / (sqrt(v) + eps)
 * (eps outside the bias correction, unlike torch.optim.Adam). */
int CassiePgAdam(int n, const float* g, float* m, float* v, float* theta, int t, float lr, float beta1, float beta2, float eps, void* stream);

/* TRPO for the 128-128 network (csrc/tu_pg_trpo.hip).  Shapes: obs_dim 26 or 17, act_dim 6 or 7 (CASSIE_EINVAL otherwise); the direction's
 * db1, dW2, db2 and dW3 must be 16-byte aligned as the weights are. */

/* CassieTrpoFvp's contract for the 128-128 network: (scale) J' S J v with J at the current weights, S = diag(prec[act_dim]) and the direction
 * dW1..db3, into partial [CassiePgPartialRows(n)][CassiePgParamCount] (rows [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], added by the caller).  Two
 * launches on `stream`: forward mode writes w = scale * prec * (J v) into work_dev [n][act_dim] (caller-owned, n * act_dim floats), then
 * CassiePgVjp takes J' w. */
int CassiePgFvp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* W3, const float* b3, const float* dW1, const float* db1, const float* dW2, const float* db2, const float* dW3,
                const float* db3, const float* prec, float scale, float* work_dev, float* partial_dev, void* stream);

/* CassieTrpoSurrogate's contract for the 128-128 network: partial [CassiePgSurrogateRows(n)][2] float64, per row
 * (sum_s -exp(ll_new - ll_old) adv_s, sum_s KL(old_s || new_s)), one row per workgroup of 128 samples; the caller adds the rows and
 * divides by the job's n. */
int CassiePgSurrogateRows(int n_samples);
int CassiePgSurrogate(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                      const float* W3, const float* b3, const float* log_std_new, const float* log_std_old, const float* act_dev,
                      const float* adv_dev, const float* old_mean_dev, double* partial_dev, void* stream);

/* CassieTrpoCgUpdate's semantics (early exit once rr' < tol, the log_std block at ls_off, reg damping) for n <= 21 504 (the 128-128
 * network has CassiePgParamCount(26, 7) + 7 = 20 878 parameters), one launch; dot products in a fixed order. */
int CassiePgCgUpdate(int n, int ls_off, int n_ls, const float* Ap_mean_dev, const float* hls_dev, float reg, float tol, float* x_dev, float* r_dev, float* p_dev,
                     float* scal_dev, void* stream);

/* ---- DDPG (cassierl_amd/ddpg.py, csrc/tu_ddpg.hip; rllab/envs/ddpg_cassie.py): 32 x 32 ReLU networks, float32, row-major as torch.nn.Linear
 * stores them.  Actor mu(s) = tanh(W3 relu(W2 relu(W1 s + b1) + b2) + b3) with W1 [32][obs_dim], W2 [32][32], W3 [act_dim][32]; critic
 * Q(s, a) = W3 relu(W2 [relu(W1 s + b1); a] + b2) + b3 with W1 [32][obs_dim], W2 [32][32 + act_dim], W3 [1][32].  A network is passed as a HOST
 * array of its six device pointers {W1, b1, W2, b2, W3, b3}.  The replay pool is a structure of arrays on the device: obs [capacity][obs_dim],
 * act [capacity][act_dim], rew [capacity], term [capacity] (0 or 1), next_obs [capacity][obs_dim].  Shapes: obs_dim 26 or 17, act_dim 6 or 7
 * (the policy step: obs_dim 26); CASSIE_EINVAL otherwise. */
#define CASSIE_DDPG_ACTOR 0
#define CASSIE_DDPG_CRITIC 1

/* parameters of the actor (which = CASSIE_DDPG_ACTOR) or the critic (CASSIE_DDPG_CRITIC); 0 for an unsupported shape */
int CassieDdpgParamCount(int obs_dim, int act_dim, int which);
/* rows of partial sums a gradient launch over `batch` samples writes (one per workgroup, at most 256) */
int CassieDdpgPartialRows(int batch);

/* One policy step for n environments in one launch (rllab's DeterministicMLPPolicy + OUStrategy + normalize()): obs float64 [n][obs_dim] ->
 *   pool_obs_row [n][obs_dim] = its float32 image;  x = path_t[i] == 0 ? ou_mu : ou_state[i];  x += ou_theta (ou_mu - x) + ou_sigma noise[i];
 *   ou_state[i] = x;  pool_act_row [n][act_dim] = clip(mu(obs) + x, -1, 1);  env_actions float64 = clip(low + (act + 1) / 2 (high - low), low, high).
 * pool_obs_row / pool_act_row point at row `top` of the pool's obs / act arrays: the caller guarantees top + n <= capacity. */
int CassieDdpgPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                         const float* b3, const float* noise_dev, const long long* path_t_dev, float ou_theta, float ou_sigma, float ou_mu, float* ou_state_dev,
                         const double* low_dev, const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream);

/* After Env.step, one launch: rew_row[i] = (float)(scale_reward * rew[i]), term_row[i] = done[i] != 0, next_obs_row = (float) next_obs, into the
 * rows the policy step opened (pointers at row `top` of the pool's rew / term / next_obs arrays). */
int CassieDdpgPoolCommit(const double* rew_dev, const unsigned char* done_dev, const double* next_obs_dev, int n, int obs_dim, double scale_reward,
                         float* pool_rew_row_dev, float* pool_term_row_dev, float* pool_next_obs_row_dev, void* stream);

/* Critic gradient on the batch idx [batch] (int64 pool rows, clamped to [0, pool_capacity)): y = rew + (1 - term) discount Q'(s', mu'(s')),
 * e = Q(s, a) - y;  partial [CassieDdpgPartialRows(batch)][CassieDdpgParamCount(critic) + 2]: gradient of SUM e^2 in the order
 * [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], then sum e^2 and sum Q(s, a). */
int CassieDdpgCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                         long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim,
                         const float* const* target_actor, const float* const* target_critic, const float* const* critic, float discount, float* partial_dev,
                         void* stream);

/* Actor gradient on the same batch: partial [rows][CassieDdpgParamCount(actor) + 1]: gradient of -SUM Q(s, mu(s)) with respect to the actor through
 * the critic as it is NOW (call it after the critic's CassieDdpgApply), then sum Q(s, mu(s)). */
int CassieDdpgActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                        const float* const* critic, float* partial_dev, void* stream);

/* One launch, one workgroup: g = scale * (the `rows` partial rows added in order);  Lasagne's Adam (CassiePgAdam's formula, t = the step count
 * after its increment) on the live network `which`;  target <- (1 - tau) target + tau live;  stats_dev[k] += the summed k-th column behind the
 * gradient (float64; 2 columns for the critic, 1 for the actor; NULL: not recorded).  m_dev / v_dev: [CassieDdpgParamCount] in the row's order. */
int CassieDdpgApply(int rows, int obs_dim, int act_dim, int which, const float* partial_dev, float scale, float* const* live, float* const* target, float* m_dev,
                    float* v_dev, int t, float lr, float beta1, float beta2, float eps, float tau, double* stats_dev, void* stream);

/* ---- SAC (cassierl_amd/sac.py, csrc/tu_sac.hip): DDPG's 32 x 32 ReLU networks, shapes and replay pool.  The actor's output layer has
 * 2 act_dim rows, W3 [2 act_dim][32]: mean = rows [0, act_dim), log_std = clamp(rows [act_dim, 2 act_dim), -20, 2); a sample is
 * u = mean + exp(log_std) eps, a = tanh(u), log pi(a|s) = sum_k (-eps_k^2 / 2 - log_std_k - log(2 pi) / 2) - sum_k 2 (log 2 - u_k - softplus(-2 u_k)).
 * The two critics are DDPG's critic: their parameter count is CassieDdpgParamCount(.., CASSIE_DDPG_CRITIC), the rows of partial sums of a batch
 * CassieDdpgPartialRows(batch), their Adam step and soft update CassieDdpgApply, the pool commit CassieDdpgPoolCommit.  The noise eps is a
 * float32 tensor [batch][act_dim] indexed by the position in the batch; the temperature is passed as a device pointer to log_alpha [1]. */

/* parameters of the actor; 0 for an unsupported shape */
int CassieSacParamCount(int obs_dim, int act_dim);

/* One policy step for n environments in one launch: obs float64 [n][obs_dim] -> pool_obs_row [n][obs_dim] = its float32 image;
 * pool_act_row [n][act_dim] = tanh(mean(obs) + exp(log_std(obs)) noise);  env_actions float64 = clip(low + (act + 1) / 2 (high - low), low, high).
 * actor: host array of the six device pointers.  pool_obs_row / pool_act_row point at row `top` of the pool: the caller guarantees top + n <= capacity. */
int CassieSacPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream);

/* Both critics' gradients on the batch idx [batch] in one launch: a' = pi(s'; eps_next),
 *   y = rew + (1 - term) discount (min(Q1', Q2')(s', a') - exp(log_alpha) log pi(a'|s')),  e_k = Q_k(s, a) - y;
 * partial [2][CassieDdpgPartialRows(batch)][CassieDdpgParamCount(critic) + 2]: block k is critic k's gradient of SUM e_k^2 in the order
 * [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], then sum e_k^2 and sum Q_k(s, a) -- the rows CassieDdpgApply(.., CASSIE_DDPG_CRITIC, ..) takes. */
int CassieSacCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream);

/* Actor gradient on the same batch: a~ = pi(s; eps); partial [rows][CassieSacParamCount + 2]: gradient of SUM (exp(log_alpha) log pi(a~|s) -
 * min(Q1, Q2)(s, a~)) with respect to the actor through the critics as they are NOW (call it after their CassieDdpgApply), then sum log pi and
 * sum min Q.  The clamp of log_std passes no gradient where it is active. */
int CassieSacActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                       const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream);

/* One launch, one workgroup: g = scale * (the `rows` partial rows added in order);  Lasagne's Adam on the actor (t = the step count after its
 * increment; there is no target actor);  log_alpha's Adam step (alpha_t likewise, its own m / v [1]) on the gradient
 * -(scale * summed log pi column + target_entropy), alpha_m_dev == NULL: the temperature stays fixed;  stats_dev[0 .. 2] += (sum log pi,
 * sum min Q, exp(log_alpha) sum log pi - sum min Q with log_alpha as it is before its step) (float64; NULL: not recorded). */
int CassieSacApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                   float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                   float target_entropy, double* stats_dev, void* stream);

/* ---- TD3 (cassierl_amd/td3.py, csrc/tu_td3.hip): DDPG's actor, two of DDPG's critics, a target of each, DDPG's shapes and replay pool.  The
 * critics' parameter count is CassieDdpgParamCount(.., CASSIE_DDPG_CRITIC), the rows of partial sums of a batch CassieDdpgPartialRows(batch), the pool
 * commit CassieDdpgPoolCommit.  The delayed actor step is CassieDdpgActorGrad with qf1 as the critic and CassieDdpgApply(.., CASSIE_DDPG_ACTOR, ..). */

/* One policy step for n environments in one launch: obs float64 [n][obs_dim] -> pool_obs_row [n][obs_dim] = its float32 image;
 * pool_act_row [n][act_dim] = clip(mu(obs) + sigma noise, -1, 1);  env_actions float64 = clip(low + (act + 1) / 2 (high - low), low, high).
 * actor: host array of the six device pointers.  pool_obs_row / pool_act_row point at row `top` of the pool: the caller guarantees top + n <= capacity.
 * obs_dim 26 only. */
int CassieTd3PolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, float sigma, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream);

/* Both critics' gradients on the batch idx [batch] (int64 pool rows, clamped to [0, pool_capacity)) in one launch:
 *   a' = clip(mu'(s') + clip(policy_noise eps_next, -noise_clip, noise_clip), -1, 1),  y = rew + (1 - term) discount min(Q1', Q2')(s', a'),
 *   e_k = Q_k(s, a) - y;
 * eps_next float32 [batch][act_dim], indexed by the position in the batch; noise_clip >= 0; policy_noise = 0 gives the unsmoothed target.
 * partial [2][CassieDdpgPartialRows(batch)][CassieDdpgParamCount(critic) + 2]: block k is critic k's gradient of SUM e_k^2 in the order
 * [gW1 | gb1 | gW2 | gb2 | gW3 | gb3], then sum e_k^2 and sum Q_k(s, a) -- CassieSacCriticGrad's layout. */
int CassieTd3CriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* target_actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, float policy_noise, float noise_clip, float discount, float* partial_dev, void* stream);

/* One launch, two workgroups: workgroup k does for critic k on block k of partial [2][rows][CassieDdpgParamCount(critic) + 2] what
 * CassieDdpgApply(.., CASSIE_DDPG_CRITIC, ..) does, bit for bit (the `rows` rows added in order, Adam with t = the step count after its increment,
 * target k <- (1 - tau) target k + tau critic k; tau = 0 leaves the target's bits);  stats_dev[0 .. 3] += (sum e_1^2, sum Q_1, sum e_2^2, sum Q_2)
 * (float64; NULL: not recorded). */
int CassieTd3CriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* qf1, float* const* qf2, float* const* target_qf1,
                         float* const* target_qf2, float* m1_dev, float* v1_dev, float* m2_dev, float* v2_dev, int t, float lr, float beta1, float beta2, float eps,
                         float tau, double* stats_dev, void* stream);

/* ---- PPO (cassierl_amd/ppo.py, csrc/tu_ppo.hip): GAE(lambda) advantages and the gradient of the clipped surrogate on a minibatch. */

/* CassieTrpoReturnsAdvantages with GAE(lambda): backwards over the T steps of an environment's column, live = !cut[s],
 *   V_next = value of the batch's own next row (last_value [n] behind the last step, NULL = 0),
 *   delta = rew[s] + gamma live V_next - value,  adv[s] = delta + gamma lambda live adv[next step]  (0 behind the last step),
 *   returns[s] as CassieTrpoReturnsAdvantages writes them (what the baseline is fitted to),
 * and partial[(n + 255) / 256][2] = per workgroup (sum adv, sum adv^2), fixed order.  lambda = 1: adv = returns - value up to rounding. */
int CassieTrpoGae(const float* obs_dev, const long long* t_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, int obs_dim,
                  const double* coeffs_dev, const double* last_value_dev, double gamma, double lambda, double* returns_dev, double* adv_dev, double* partial_dev,
                  void* stream);

/* Gradient of PPO's clipped surrogate on one minibatch, one launch: the forward pass of the mean network at the GIVEN weights on the m rows
 * idx [m] of the batch (int64, clamped to [0, n); NULL = rows 0 .. m - 1, m <= n), then in registers
 *   ratio = exp(ll_new(act) - ll_old(act)),  clipped = (adv > 0 and ratio > 1 + clip) or (adv < 0 and ratio < 1 - clip),  w = clipped ? 0 : ratio adv,
 *   d L / d mean = -scale w z / std  (z = (act - mean) / std at the given weights and log_std_new),
 * then the reverse pass of CassieTrpoVjp / CassiePgVjp.  obs [n][obs_dim], act / old_mean [n][act_dim], adv [n] are indexed by batch row;
 * log_std_old / log_std_new [act_dim].  partial [rows][ParamCount + act_dim] float32 = [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | g_log_std] with
 * g_log_std = -scale sum_s w (z^2 - 1) (an entropy bonus is a constant the caller adds); stats [rows][3] float64 = per row
 * (sum_s -min(ratio adv, clip(ratio, 1 - clip, 1 + clip) adv), sum_s KL(old_s || new_s), number of clipped samples).  The caller adds the
 * rows: CassieTrpoClipGradRows(m) of them, one per wavefront (width 32), CassiePgClipGradRows(m), one per workgroup (width 128, whose b1, W2,
 * b2, W3 must be 16-byte aligned).  Every sum runs in a fixed order: a call repeats bit for bit. */
int CassieTrpoClipGradRows(int m);
int CassieTrpoClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                       const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                       double* stats_dev, void* stream);
int CassiePgClipGradRows(int m);
int CassiePgClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                     const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                     double* stats_dev, void* stream);

/* ---- width-128 policy at 45 x 10: PPO on Cassie3d (cassierl_amd/ppo.py with env="cassie3d", csrc/tu_pg3d.hip).  The contracts of
 * CassiePgParamCount, CassiePgPolicyStep, CassiePgClipGradRows and CassiePgClipGrad for the one shape obs_dim = 45, act_dim = 10 (any other:
 * 0 / CASSIE_EINVAL); Adam is CassiePgAdam.  The baseline kernels above take obs_dim = 45 (94 features) under their own names. */
int CassiePg3dParamCount(int obs_dim, int act_dim);
int CassiePg3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2,
                         const float* b2, const float* W3, const float* b3, const float* log_std, const float* noise_dev,
                         const double* low_dev, const double* high_dev, float* obs32_dev, float* mean_dev, float* act_dev,
                         double* env_actions_dev, void* stream);
int CassiePg3dClipGradRows(int m);
int CassiePg3dClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                       const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                       double* stats_dev, void* stream);

/* ---- value network: PPO's learned V(s) (cassierl_amd/value.py, csrc/tu_vf.hip), the 128 x 128 tanh network of the width-128 policy with ONE
 * output row -- W1 [128][obs_dim], b1 [128], W2 [128][128], b2 [128], W3 [1][128], b3 [1], float32, row-major as torch.nn.Linear, b1 / W2 / b2 / W3
 * 16-byte aligned -- for obs_dim 26 (Cassie2d) and 45 (Cassie3d).  Any other shape: CassieVfParamCount is 0 and the launchers return CASSIE_EINVAL;
 * so does a null pointer, n / m / T <= 0 or a misaligned pointer, before anything is launched or written.  Adam is CassiePgAdam.  Every sum runs
 * in a fixed order: a call repeats bit for bit. */
int CassieVfParamCount(int obs_dim);   /* 128 obs_dim + 128 + 128^2 + 128 + 128 + 1, or 0 */

/* value[i] = V(obs[i]) for i < n (obs [n][obs_dim] float32), one launch; rows past n are untouched. */
int CassieVfPredict(const float* obs_dev, int n, int obs_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                    const float* b3, float* value_dev, void* stream);

/* CassieTrpoGae with the value of every sample READ from values [T][n] (float32, promoted) instead of evaluated, last_value [n] float32 (NULL = 0),
 * and the value target vtarget[s] = adv[s] + values[s] (the lambda-return, evaluated by its own recurrence y_t = r_t + gamma live_t ((1 - lambda)
 * v_{t+1} + lambda y_{t+1}), which does not cancel where |values| is far above the return) beside returns and adv; partial[(n + 255) / 256][2] =
 * (sum adv, sum adv^2). */
int CassieVfGae(const float* values_dev, const float* last_value_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, double gamma,
                double lambda, double* returns_dev, double* adv_dev, double* vtarget_dev, double* partial_dev, void* stream);

/* Gradient of the value loss (1 / 2M) sum_i (V(s_i) - target_i)^2 on one minibatch, one launch: the rows idx [m] of the batch (int64, clamped to
 * [0, n); NULL = rows 0 .. m - 1, m <= n), the forward pass at the GIVEN weights, the cotangent scale (V - target[row]) in registers (scale = 1 / M),
 * the reverse pass of CassiePgVjp.  target [n] is indexed by batch row.  partial [rows][ParamCount] float32 = [gW1 | gb1 | gW2 | gb2 | gW3 | gb3],
 * stats [rows] float64 = sum_s (V - target)^2 / 2; rows = CassieVfGradRows(m), one per workgroup; the caller adds the rows. */
int CassieVfGradRows(int m);
int CassieVfGrad(const float* obs_dev, int n, int obs_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                 const float* b3, const long long* idx_dev, int m, const float* target_dev, float scale, float* partial_dev, double* stats_dev, void* stream);

/* ---- SAC at 45 x 10: Soft Actor-Critic on Cassie3d (cassierl_amd/sac.py with env="cassie3d", csrc/tu_sac3d.hip on the kernels of csrc/sac_kernels.h).  The networks
 * are still the 32 x 32 ReLU networks above: the actor's W1 [32][45], W3 [20][32] (mean rows [0, 10), log_std rows [10, 20)), a critic's W1 [32][45],
 * W2 [32][42].  The contracts of CassieSacPolicyStep, CassieSacCriticGrad, CassieSacActorGrad and CassieSacApply (here CassieSac3dActorApply) for the
 * one shape obs_dim = 45, act_dim = 10; any other shape, a null pointer, batch / n / rows <= 0 or a misaligned pointer is CASSIE_EINVAL before
 * anything is launched.  CassieDdpgApply and CassieSacApply keep refusing this shape: a critic's Adam step and soft update is
 * CassieSac3dCriticApply (CassieDdpgApply's contract for the critic, 2 statistics columns).  The rows of partial sums of a batch are
 * CassieDdpgPartialRows(batch), the pool commit is CassieDdpgPoolCommit (both shape-free).  One update is five launches: CassieSac3dCriticGrad,
 * CassieSac3dCriticApply for each critic, CassieSac3dActorGrad, CassieSac3dActorApply.  Every sum runs in a fixed order: a call repeats bit for bit. */

/* parameters of the actor (which = CASSIE_DDPG_ACTOR: 3188) or of a critic (CASSIE_DDPG_CRITIC: 2881); 0 for any other shape.  Host only. */
int CassieSac3dParamCount(int obs_dim, int act_dim, int which);
int CassieSac3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                          const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream);
/* partial [2][CassieDdpgPartialRows(batch)][2881 + 2] */
int CassieSac3dCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                          long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                          const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                          const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream);
/* partial [CassieDdpgPartialRows(batch)][3188 + 2] */
int CassieSac3dActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                         const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream);
/* One launch, one workgroup, on one critic's block [rows][2881 + 2]: g = scale * (the rows added in order);  Adam on `live` (t = the step count after
 * its increment);  target <- (1 - tau) target + tau live;  stats_dev[0 .. 1] += (sum e^2, sum Q) (float64; NULL: not recorded). */
int CassieSac3dCriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* live, float* const* target, float* m_dev,
                           float* v_dev, int t, float lr, float beta1, float beta2, float eps, float tau, double* stats_dev, void* stream);
int CassieSac3dActorApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                          float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                          float target_entropy, double* stats_dev, void* stream);

/* ---- ES (cassierl_amd/es.py, csrc/tu_es.hip): antithetic perturbations of the 32 x 32 tanh mean network drawn from a shared noise table.
 * theta [P] is the mean network's parameter row [W1 | b1 | W2 | b2 | W3 | b3] (row-major as torch.nn.Linear), P = CassieEsParamCount; table
 * [table_len] float32 holds standard normal numbers; direction d is eps_d = table[offsets[d] : offsets[d] + P].  Environment i evaluates
 * direction i >> 1 with sign +1 (i even) or -1 (i odd).  Every offset must lie in [0, table_len - P] (CassieEsGrad: table_len - n_params):
 * the kernels do NOT check them (cassierl_amd/es.py: EsKernels.set_directions does, on the host, before anything is launched). */

/* parameters of the mean network, as CassieTrpoParamCount; 0 for an unsupported shape (supported: obs_dim 26 or 17, act_dim 6 or 7) */
int CassieEsParamCount(int obs_dim, int act_dim);
/* pairs of environments that one workgroup of CassieEsPolicyStep evaluates (its grid is ceil(n / 2 / this)) */
int CassieEsPairsPerWorkgroup(void);

/* One policy step of the whole population in ONE launch; n even, obs float64 [n][obs_dim] as the environment wrote it:
 *   w_i = theta + (s_i sigma) eps_(i >> 1),  mean_i = W3 tanh(W2 tanh(W1 obs_i + b1) + b2) + b3 with the layers cut out of w_i,
 *   act_i = alive[i] ? mean_i : 0  (alive NULL: every environment is alive),
 *   env_actions float64 [n][act_dim] = clip(low + (act + 1) / 2 * (high - low), low, high): a dead environment gets the middle of the box.
 * A pair with both environments dead reads nothing from the table.  Nothing but env_actions[0 : n] is written; a call repeats bit for bit.
 * CASSIE_EINVAL: odd n, table_len < P, a null pointer (other than alive), an unsupported shape. */
int CassieEsPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                       const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                       double* env_actions_dev, void* stream);

/* The same three for the 128 x 128 tanh mean network (csrc/tu_es_wide.hip): P = 128 D + 128 + 128 * 128 + 128 + 128 A + A for the shapes above
 * (20 742 for (26, 6)), 0 for any other shape; CassieEsWidePolicyStep has CassieEsPolicyStep's arguments, contract and return codes, with this P.
 * The pair's slice of the table is streamed in chunks through LDS, every entry read once; CassieEsBook and CassieEsGrad serve both widths. */
int CassieEsWideParamCount(int obs_dim, int act_dim);
int CassieEsWidePairsPerWorkgroup(void);
int CassieEsWidePolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                           const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                           double* env_actions_dev, void* stream);

/* ---- ES at 45 x 10 (csrc/tu_es3d.hip): the same six for Cassie3d's shape, obs_dim 45 and act_dim 10, the one shape they take.
 * CassieEs3dParamCount is 2858 (32 x 32) and CassieEs3dWideParamCount 23 690 (128 x 128) for (45, 10), 0 for any other shape; the two policy steps
 * have CassieEsPolicyStep's arguments, contract and return codes with these P.  CassieEsParamCount and CassieEsWideParamCount stay 0 at (45, 10):
 * the shape lives behind these symbols only.  CassieEsBook and CassieEsGrad serve this shape as they are. */
int CassieEs3dParamCount(int obs_dim, int act_dim);
int CassieEs3dPairsPerWorkgroup(void);
int CassieEs3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                         const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                         double* env_actions_dev, void* stream);
int CassieEs3dWideParamCount(int obs_dim, int act_dim);
int CassieEs3dWidePairsPerWorkgroup(void);
int CassieEs3dWidePolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                             const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                             double* env_actions_dev, void* stream);

/* Bookkeeping of one Env.step of the population in one launch, with rew / done as CassieVecStep wrote them:
 *   fitness[i] += alive[i] ? rew[i] : 0;  length[i] += alive[i];  alive[i] &= !done[i]   (alive: one byte, 0 / 1). */
int CassieEsBook(const double* rew_dev, const unsigned char* done_dev, int n, unsigned char* alive_dev, double* fitness_dev, long long* length_dev, void* stream);

/* The weighted sum of m directions: partial [rows][n_params] float32, rows = CassieEsGradRows(m);
 *   partial[r][k] = sum over the directions d of row r, ascending, of w[d] table[offsets[d] + k]   (a float32 fmaf chain from 0),
 * row r holding the directions [r c, min(m, (r + 1) c)), c = ceil(m / rows) (a row past m is all zero).  Any n_params >= 1.  The caller adds the
 * rows; a call repeats bit for bit. */
int CassieEsGradRows(int m);
int CassieEsGrad(const float* table_dev, long long table_len, const long long* offsets_dev, const float* w_dev, int m, int n_params, float* partial_dev,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
