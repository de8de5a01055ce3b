/*
 * sparenet_hip.h -- C ABI of libsparenet_hip.so, the MI355X (gfx950) native
 * implementation of SpareNet's per-step loss / render hot path.
 *
 * Drop-in boundary: each entry point replaces one pybind function of the
 * reference's torch C++ extensions under /root/reference/cuda/ (cited per
 * function as file:line).  No torch types cross this boundary: every argument
 * is a raw DEVICE pointer (hipMalloc'ed / torch CUDA-tensor storage), an int
 * size or a float parameter, plus the hipStream_t (as void*) to launch on.
 *
 * Conventions
 *   - all tensors are contiguous row-major fp32 / int32, sizes in elements;
 *   - functions are asynchronous: they enqueue kernels on `stream` and return;
 *   - return value: 0 (hipSuccess) on success; a positive hipError_t if a
 *     launch failed; SN_EINVAL (-22) for rejected arguments (the reference
 *     prints and carries on, asserts in Python or exit(-1)s; here every
 *     failure is an error code + sn_last_error() text, and the Python mirror
 *     raises);
 *   - workspace: ops that need scratch take (workspace, workspace_bytes); the
 *     matching sn_*_workspace_bytes() says how much.  Each workspace is defined
 *     by ONE layout function next to its entry point (sn::Carver in
 *     sparenet_amd/csrc/common.hpp): the size export measures that layout, the
 *     entry point carves it and checks workspace_bytes against it.  Workspace
 *     contents need no initialisation by the caller;
 *   - thread safety: no global mutable state except the thread-local
 *     last-error string; safe to call concurrently from several host threads
 *     on different streams/devices (the reference is driven that way by
 *     nn.DataParallel, runners/sparenet_runner.py:32-34).
 */
#ifndef SPARENET_HIP_H
#define SPARENET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_EINVAL (-22)
/* a team barrier of an earlier persistent EMD launch on this device gave up (see sn_emd_forward) */
#define SN_ETIMEDOUT (-110)
#define SN_ABI_VERSION 4

int sn_abi_version(void);
/* hash of the HIP sources this library was built from (profiles/ measurements carry it) */
const char *sn_build_id(void);
/* thread-local text of the last failure on the calling thread ("" if none) */
const char *sn_last_error(void);
/* 0, or SN_ETIMEDOUT if a bounded wait inside an earlier multi-workgroup launch (persistent EMD auction, density
 * sampler teams) on the CURRENT device gave up; clears the condition.  No synchronisation (one word of pinned host
 * memory is read): call it where the host already waits for the GPU -- after reading a loss value -- to learn about
 * a time-out in the step that just finished instead of at the next sn_emd_* / sn_mds call. */
int sn_device_status(void);

/* Wait policy of the two ops whose workgroups wait for each other inside one launch (the persistent EMD auction's
 * teams, the density sampler's teams).  On a device shared with another process a team can lose compute units to it
 * and give up after its bounded spin:
 *   SN_WAIT_FAIL    (default) the unfinished clouds come back as NaN / -1 rows and the device's sticky word makes the
 *                   next sn_emd_* / sn_mds call (or sn_device_status) return SN_ETIMEDOUT;
 *   SN_WAIT_RECOVER teams as by default, but a team that gives up leaves the sticky word alone: the same call
 *                   recomputes its clouds on the same stream with kernels that wait for nobody (exact: the same
 *                   results as a call that never timed out) and counts them.  Once a recovery has been seen on a
 *                   device (the counters of sn_wait_report grew) later calls there take the non-waiting path
 *                   directly (the "latch", cleared by sn_set_wait_policy);
 *   SN_WAIT_NOWAIT  never launch a team-waiting kernel: the auction runs with teams of one workgroup, the sampler with
 *                   its one-workgroup kernel.
 * The policy is process-wide; SN_WAIT_POLICY=fail|recover|nowait in the environment gives its initial value.
 * sn_set_wait_policy returns SN_EINVAL for any other value.  sn_wait_report writes the first min(n, 3) of: EMD clouds
 * recovered on the current device, sampler clouds recovered there, 1 if the device's latch is set; like
 * sn_device_status it reads pinned host words without a synchronisation (meaningful for work that has finished). */
#define SN_WAIT_FAIL 0
#define SN_WAIT_RECOVER 1
#define SN_WAIT_NOWAIT 2
int sn_set_wait_policy(int policy);
int sn_wait_policy(void);
int sn_wait_report(long long *out, int n);

/* Optional per-kernel timing, off by default (measurement aid, not part of the
 * reference interface): when enabled the heavy kernels ("chamfer_fwd", "emd_auction",
 * "expansion_fwd", "mds", "p2i_max_splat" = the binned gather) are bracketed by hipEventRecord on the
 * stream they are launched on.  sn_prof_read waits for the recorded events and returns
 * the number of launches of `name` since the last reset and their summed duration. */
void sn_prof_enable(int on);
long long sn_prof_read(const char *name, double *total_ms);
void sn_prof_reset(void);
/* With sn_prof_enable(1) the persistent EMD auction also records its own EXECUTION window (first working workgroup's
 * start to the last one's end, in-kernel 100 MHz clock): launches since the last reset on the current device and the
 * sum of the windows.  The HIP-event bracket of "emd_auction" additionally contains the launch's wait for compute
 * units (the grid needs every CU empty), i.e. the schedule around it. */
long long sn_emd_prof_exec(double *total_ms, int reset);

/* ------------------------------------------------------------------ Chamfer
 * replaces cd.forward_cuda  = chamfer_distance_forward_cuda
 *          (cuda/chamfer_distance/chamfer_distance.cpp:26-38,186;
 *           kernel chamfer_distance.cu:7-155)
 * dist1[b,j] = min_k |xyz1[b,j]-xyz2[b,k]|^2, idx1 = lowest k attaining it;
 * symmetric for dist2/idx2.  b>=1, n>=1, m>=1. */
int sn_chamfer_forward(const float *xyz1, const float *xyz2, int b, int n,
                       int m, float *dist1, int *idx1, float *dist2,
                       int *idx2, void *stream);
/* replaces cd.backward_cuda = chamfer_distance_backward_cuda
 *          (chamfer_distance.cpp:40-55,188; kernel chamfer_distance.cu:159-209)
 * gradxyz1/gradxyz2 are fully overwritten (no pre-zeroing needed).  The scatter of the reference is a
 * gather over inverse lists built in `workspace` (integer atomics only): the result is bit-reproducible and
 * bit-equal to the reference's CPU path, which adds the same terms in the same order. */
/* Same result as sn_chamfer_forward (distances bit for bit, indices = lowest k attaining the
 * minimum), computed as a spatially pruned search: both clouds are Morton sorted into the
 * workspace, superblocks of 64 targets are skipped by bounding box, the surviving pairs are
 * filtered on the fp32 matrix cores and only the candidates are evaluated with the reference's
 * expression.  Pays off from a few thousand points per cloud. */
size_t sn_chamfer_workspace_bytes(int b, int n, int m);
int sn_chamfer_forward_sorted(const float *xyz1, const float *xyz2, int b, int n,
                              int m, float *dist1, int *idx1, float *dist2,
                              int *idx2, void *workspace, size_t workspace_bytes,
                              void *stream);
size_t sn_chamfer_backward_workspace_bytes(int b, int n, int m);
int sn_chamfer_backward(const float *xyz1, const float *xyz2,
                        const float *graddist1, const float *graddist2,
                        const int *idx1, const int *idx2, int b, int n, int m,
                        float *gradxyz1, float *gradxyz2, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Host tensors (replaces cd.forward / cd.backward = chamfer_distance_forward / chamfer_distance_backward,
 * chamfer_distance.cpp:91-180,185,187 -- the branch ChamferDistanceFunction takes for CPU tensors,
 * cuda/chamfer_distance/chamfer_distance.py:31-32,53-54; BASELINE config 1).  All pointers are HOST pointers, the
 * calls are synchronous.  Same values as the device entry points and as the reference's CPU code bit for bit: fp32
 * distances (dx*dx + dy*dy) + dz*dz without contraction, lowest index among equal minima, the backward's additions in
 * the reference's order.  threads: worker threads; an explicit value > 0 is taken as given.  0 = the default: one per
 * hardware thread, or SN_HOST_THREADS when set -- the default (either form) is then reduced so that every thread
 * has at least four work items (clouds x query blocks).  Never more than 256, never more than there are items.
 * The library's own host code, not a fallback: device tensors never take this path. */
int sn_chamfer_forward_host(const float *xyz1, const float *xyz2, int b, int n,
                            int m, float *dist1, int *idx1, float *dist2,
                            int *idx2, int threads);
int sn_chamfer_backward_host(const float *xyz1, const float *xyz2,
                             const float *graddist1, const float *graddist2,
                             const int *idx1, const int *idx2, int b, int n, int m,
                             float *gradxyz1, float *gradxyz2, int threads);

/* ---------------------------------------------------------------------- EMD
 * replaces emd.forward = emd_forward -> emd_cuda_forward
 *          (cuda/emd/emd.cpp:13-17,26; emd_cuda.cu:228-282) including the 12
 *          scratch tensors the Python module allocates and initialises
 *          (cuda/emd/emd_module.py:43-54): they live in `workspace` here.
 * Requirements as the reference: n % 1024 == 0, b <= 512 (emd_module.py:36-39).
 * dist[b,n] fp32, assignment[b,n] int32.
 * All iterations run in ONE persistent launch (one workgroup per compute unit; teams of
 * workgroups own a cloud and synchronise through bounded, placement-independent barriers).
 * Environment: SN_EMD_CHECK=1 makes the call synchronise and fail if a barrier timed out (under SN_WAIT_RECOVER: if
 * a time-out survived the recovery pass).
 * SN_EMD_RETIRE (read once per process; results are bit-identical for every value): the unassigned bidders per
 * workgroup (cloud total / workgroups of the team) from which on every workgroup of a team's LAST cloud ends waves
 * 8-15 and frees half of its compute unit's registers for kernels of other streams -- unset: 80, and only in launches
 * whose teams all have a cloud; 0: never; a positive value: that threshold in every launch; -k-1: at the top of
 * iteration k whatever the cloud looks like (tests and experiments).  Contested and far clouds never retire on their own.
 * stats (optional device pointer, may be NULL): 2 x int64, zeroed by the caller
 *   stats[0] += sum over iterations and batch of unassigned_count * n
 *               (effective pair evaluations); stats[1] += iterations that had
 *               at least one bidder (one atomic per cloud per iteration).
 *   In a call that recovered clouds (SN_WAIT_RECOVER) both also hold the iterations the abandoned team launch had
 *   done before it gave up, on top of the recovery's complete run of those clouds.
 * With SN_EMD_DIAG=1|2 in the environment the call also leaves phase timers of the first team
 * in the workspace, 16 + 64*64 int64 words at sn_emd_diag_offset (tools/emd_ab.py).
 *
 * Failure behaviour (the reference returns an error code from emd_cuda_forward, emd_cuda.cu:276-281): the
 * auction is ONE persistent launch whose workgroups wait for each other; every wait is bounded (> 2 s).  If a
 * barrier gives up (a CU withheld from the launch by another tenant or a debugger), every workgroup leaves and
 * the unfinished clouds get dist = NaN and assignment = -1.  Then, by the wait policy (sn_set_wait_policy):
 *   fail (default): the NEXT sn_emd_forward / sn_emd_backward call on that device returns SN_ETIMEDOUT without a
 *     host synchronisation (SN_EMD_CHECK=1: the failing call itself synchronises and returns SN_EINVAL);
 *   recover: a recovery pass enqueued behind the launch (no host synchronisation) picks the NaN / -1 clouds on the
 *     device, redoes their set-up and runs their auction with teams of one workgroup; the result is bit-identical
 *     to a call that never timed out, and sn_wait_report counts the clouds.  Without a time-out the pass costs one
 *     small launch and three launches whose workgroups leave at once;
 *   nowait: teams of one workgroup from the start (no workgroup waits for another).
 * Memory-model note: the launch hands data between workgroups with relaxed coherent accesses and no fences, and
 * keeps the stores of a team that sits on one XCD in that XCD's L2.  This is gfx950 behaviour, verified once per
 * device by a litmus kernel at the first call; on failure, or with SN_EMD_SAFE=1, the launch uses agent-scope
 * release / acquire barriers and agent-scope stores instead (sn_emd_mode() reports which). */
size_t sn_emd_workspace_bytes(int b, int n);
size_t sn_emd_diag_offset(int b, int n);
int sn_emd_mode(void);
/* runs the memory-model litmus of the current device now (what the first sn_emd_forward does lazily, on a private
 * stream, without a device-wide synchronisation) and returns sn_emd_mode()'s answer; -1: undecided (busy device). */
int sn_emd_selftest(void);
int sn_emd_forward(const float *xyz1, const float *xyz2, int b, int n,
                   float eps, int iters, float *dist, int *assignment,
                   void *workspace, size_t workspace_bytes,
                   long long *stats, void *stream);
/* replaces emd.backward = emd_backward -> emd_cuda_backward
 *          (cuda/emd/emd.cpp:19-23,27; emd_cuda.cu:284-316)
 * gradxyz1 is fully overwritten; gradient w.r.t. xyz2 is identically zero. */
int sn_emd_backward(const float *xyz1, const float *xyz2,
                    const float *graddist, const int *assignment, int b, int n,
                    float *gradxyz1, void *stream);

/* ------------------------------------------------------- EMD, any size n <= m
 * The auction above for clouds of any size: xyz1[b,n,3] are the bidders, xyz2[b,m,3] the targets, 1 <= n <= m <= 2^20,
 * b >= 1 (<= 65535).  dist[b,n] fp32, assignment[b,n] int32 (index into the cloud's m targets).  Per cloud and
 * iteration, with cnt = the cloud's unassigned bidders:
 *   block_cnt = ceil(n / 1024), unass_per_block = ceil(cnt / block_cnt), tpu = 1024 / unass_per_block;
 *   Bid: a bidder scans the m targets in tiles of 2048, thread t of its tpu threads owning the contiguous chunk t of
 *     every tile (delta = ceil(tile length / tpu)); d_k = (float)((3.0 - (double)sqrtf(s)) - (double)price[k]),
 *     s = (dx*dx + dy*dy) + dz*dz rounded per operation, dx = target - query; best = max d, better = the second
 *     element of the descending multiset of values (an exact tie gives better == best; both start at -1e9, so with
 *     m = 1 better stays -1e9); best_i = argmin (thread(k), k) among the maximal values; increment =
 *     (best - better) + eps, and the target's max_increment becomes the maximum of itself and the increments bid on it;
 *   GetMax: among the bidders whose increment bi satisfies bi - 1e-6 <= mi <= bi + 1e-6 (double compare; mi = the
 *     target's max_increment) the highest j writes max_idx[target].  max_idx is NOT cleared between iterations and
 *     starts at 0, max_increment starts at 0;
 *   Assign: a bidder with max_idx[target] == j -- every bidder in the last iteration -- takes its target (outside the
 *     last iteration evicting its owner), price[target] += increment, max_increment[target] = -1e9;
 *   CalcDist: dist[j] = (dx*dx + dy*dy) + dz*dz, dx = xyz1[j] - xyz2[assignment[j]]; with iters == 0 every
 *     assignment is -1 and every dist 0.
 * For n == m, n % 1024 == 0 this is exactly sn_emd_forward's contract, and such calls with b <= 512 ARE handed to
 * sn_emd_forward (the persistent auction) unless SN_EMD_GENERAL=1 is set; every other call runs ordinary stream-ordered
 * launches (three per iteration) in which no workgroup waits for another: no team, no time-out, no wait policy.
 * stats as in sn_emd_forward (stats[0] += cnt * m per cloud and iteration).  Refused with SN_EINVAL: n > m (pass the
 * smaller cloud first), m > 2^20, b < 1, a workspace smaller than sn_emd_general_workspace_bytes(b, n, m) (0 for
 * invalid sizes). */
size_t sn_emd_general_workspace_bytes(int b, int n, int m);
int sn_emd_forward_general(const float *xyz1, const float *xyz2, int b, int n, int m,
                           float eps, int iters, float *dist, int *assignment,
                           void *workspace, size_t workspace_bytes,
                           long long *stats, void *stream);
/* gradxyz1[j] = 2 graddist[j] (xyz1[j] - xyz2[a(j)]) (the formula of sn_emd_backward), 0 where a(j) = -1 (or out of
 * range); gradxyz2 (nullable; then workspace may be NULL) [b,m,3]: gradxyz2[k] = ((0 - t_j1) - t_j2) - ... in fp32 over
 * the bidders j1 < j2 < ... with a(j) = k, t_j = gradxyz1[j]; 0 for a target nobody holds.  Several bidders share a
 * target only through the last iteration's forced assignment (all but one of a group of identical bidders, for
 * instance).  Both results are bit-reproducible; the work is linear in n + m however the bidders share targets.  The
 * workspace is sized by sn_emd_general_backward_workspace_bytes(b, n, m) (0 for invalid sizes). */
size_t sn_emd_general_backward_workspace_bytes(int b, int n, int m);
int sn_emd_backward_general(const float *xyz1, const float *xyz2, const float *graddist,
                            const int *assignment, int b, int n, int m, float *gradxyz1,
                            float *gradxyz2, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ------------------------------------------------------------ ragged batches
 * Chamfer and EMD for a batch whose clouds have different numbers of points.
 *
 * Contract.  A ragged batch is a dense fp32 tensor [b, n, 3] plus lengths[b] (int32, a DEVICE pointer like every other
 * pointer here): the first lengths[i] rows of cloud i are its points, the rest is padding, 0 <= lengths[i] <= n (a value
 * outside is held to that range, or makes an EMD cloud invalid: no length can address memory outside the cloud's rows).
 *   - a padding row's value is never read into any result, NaN and Inf included;
 *   - for a padding row distances are 0, indices and assignments -1, gradients 0;
 *   - a cloud's valid rows get exactly what the dense entry point gives for that cloud alone (b = 1, the arrays cut to
 *     its lengths), bit for bit: distances, indices, assignments and gradients.  The other clouds of the batch, their
 *     lengths and the padded width n have no influence;
 *   - Chamfer with an empty side (lengths1[i] == 0 or lengths2[i] == 0): the cloud's distances are 0, its indices -1
 *     and its gradients 0, on both sides;
 *   - EMD with lengths1[i] == 0 or lengths1[i] > lengths2[i] (an invalid cloud): its whole dist row is NaN, its
 *     assignment row -1 and its gradients 0; no kernel touches the cloud's points.
 * Every entry point runs on the caller's stream as ordinary launches, reads the lengths on the device only (no host
 * synchronisation), and has no workgroup wait for another: no wait policy applies.  n and m below are the padded
 * widths = the row strides of every array; grids are sized for them, and work past a cloud's length leaves at once.
 *
 * sn_pad_compact turns the reference's padding convention (cuda/chamfer_dist/__init__.py:27-31,
 * cuda/gridding/__init__.py:41-47: a row whose coordinates sum to zero is padding) into this contract: per cloud the
 * rows with (x + y) + z != 0 -- fp32, in this order, the expression sn_gridding_forward_padded applies; a NaN sum
 * keeps the row -- move to the front of packed[b,n,3] in their order (a stable partition; one workgroup per cloud, any
 * n), lengths[b] counts them, src[b,n] holds the original row of every packed row and -1 beyond the length, where
 * packed is 0.  packed must not alias xyz.
 * sn_pad_scatter_rows is its inverse for per-row values (the backward pass): rows[b,n,c] -> out[b,n,c] with
 * out[i, src[i,p], :] = rows[i, p, :] for src[i,p] >= 0 and 0 in every other row; out is fully overwritten. */
int sn_pad_compact(const float *xyz, int b, int n, float *packed, int *lengths, int *src, void *stream);
int sn_pad_scatter_rows(const float *rows, const int *src, int b, int n, int c, float *out, void *stream);
/* sn_chamfer_forward's all-pairs kernel with per-cloud query and target counts: xyz1[b,n,3] with lengths1[b],
 * xyz2[b,m,3] with lengths2[b]; dist1/idx1 [b,n], dist2/idx2 [b,m], fully overwritten. */
int sn_chamfer_forward_ragged(const float *xyz1, const float *xyz2, int b, int n, int m,
                              const int *lengths1, const int *lengths2, float *dist1, int *idx1,
                              float *dist2, int *idx2, void *stream);
/* sn_chamfer_backward over the valid rows: the inverse lists hold valid rows only and are summed in the same ascending
 * order, lists longer than 64 entries (collapsed predictions) by a workgroup as there.  gradxyz1 / gradxyz2 fully
 * overwritten.  graddist values at padding rows are not read. */
size_t sn_chamfer_backward_ragged_workspace_bytes(int b, int n, int m);
int sn_chamfer_backward_ragged(const float *xyz1, const float *xyz2, const float *graddist1,
                               const float *graddist2, const int *idx1, const int *idx2, int b, int n, int m,
                               const int *lengths1, const int *lengths2, float *gradxyz1, float *gradxyz2,
                               void *workspace, size_t workspace_bytes, void *stream);
/* The stream-ordered auction of sn_emd_forward_general with n_i = lengths1[i] bidders and m_i = lengths2[i] targets per
 * cloud: block_cnt = ceil(n_i / 1024) and tpu come from the cloud's own n_i.  The padded widths need not satisfy
 * n <= m (1 <= n, m <= 2^20).  Never handed to the persistent auction, whatever the shapes.  dist / assignment [b,n];
 * stats as in sn_emd_forward_general (stats[0] += cnt * m_i).  The backward is sn_emd_backward_general's (gradxyz2
 * nullable, an ascending-j fp32 sum per target); rows beyond lengths1[i] and invalid clouds count as unassigned
 * whatever `assignment` holds there, and their graddist is not read. */
size_t sn_emd_ragged_workspace_bytes(int b, int n, int m);
int sn_emd_forward_ragged(const float *xyz1, const float *xyz2, int b, int n, int m, const int *lengths1,
                          const int *lengths2, float eps, int iters, float *dist, int *assignment,
                          void *workspace, size_t workspace_bytes, long long *stats, void *stream);
size_t sn_emd_ragged_backward_workspace_bytes(int b, int n, int m);
int sn_emd_backward_ragged(const float *xyz1, const float *xyz2, const float *graddist,
                           const int *assignment, int b, int n, int m, const int *lengths1,
                           const int *lengths2, float *gradxyz1, float *gradxyz2, void *workspace,
                           size_t workspace_bytes, void *stream);

/* -------------------------------------------------------- expansion penalty
 * replaces expansion_penalty.forward = expansion_penalty_forward
 *          (cuda/expansion_penalty/expansion_penalty.cpp:8-12,20;
 *           expansion_penalty_cuda.cu:7-165) without the two [b, n*512]
 *          neighbor/cost scratch tensors
 *          (expansion_penalty_module.py:33-34).
 * primitive_size: power of two, 2..512, n % primitive_size == 0.
 * mean_mst_length[b] = sum over patches (ascending patch order) of the patch's
 * mean MST edge length, UN-normalised exactly like the reference kernel leaves
 * it; expansion_penalty_module.py:40 divides by n/primitive_size in Python and
 * the host mirror does the same. */
size_t sn_expansion_workspace_bytes(int b, int n, int primitive_size);
int sn_expansion_forward(const float *xyz, int b, int n, int primitive_size,
                         float alpha, float *dist, int *assignment,
                         float *mean_mst_length, void *workspace,
                         size_t workspace_bytes, void *stream);
/* replaces expansion_penalty.backward (expansion_penalty.cpp:14-17,21;
 *          expansion_penalty_cuda.cu:167-198); gradxyz fully overwritten. */
int sn_expansion_backward(const float *xyz, const float *graddist,
                          const int *assignment, int b, int n, float *gradxyz,
                          void *stream);

/* ---------------------------------------------------------------------- MDS
 * replaces MDS.minimum_density_sampling (cuda/MDS/MDS.cpp:114-135,140;
 *          kernel MDS_cuda.cu:91-268).  idx[b,m] int32, m <= n.
 * The `temp` tensor MDS.cpp:119-121 allocates lives in registers; only clouds
 * with more than 24576 points need `workspace` (sn_mds_workspace_bytes() > 0).
 * The density kernel is sn_expf (include/sn_expf.h), not libm/OCML expf.
 * Degenerate mean_mst_length (a collapsed coarse cloud): t = (float)(5 mml^2) may be 0 or subnormal.  -d/t is then
 * evaluated as a correctly rounded IEEE quotient (no reciprocal shortcut): -inf for d > 0 and NaN for d = 0 when
 * t = 0, and sn_expf(-inf) = sn_expf(NaN) = 0, so every density stays 0 and the tie order alone -- arg-min of
 * (bitrev(k mod bs), k) -- picks the points.  (The reference's expf(NaN) = NaN poisons the density of every duplicate
 * of the last pick instead; its order there is not reproduced.)  Clouds of 2048 .. 19456 points are cluster-sorted and sampled either by one workgroup each or by a TEAM of up to
 * 32 workgroups per cloud that takes several exact picks per exchange (every cloud of >= 8192 points when teams of
 * >= 8 fit the device; index sequences are the reference's either way).  A team's bounded waits can give up when the
 * device is shared with something that keeps compute units from the launch; the cloud's row is then -1, and by the
 * wait policy (sn_set_wait_policy):
 *   fail (default): the next sn_mds / sn_emd_* call -- or sn_device_status() -- reports SN_ETIMEDOUT;
 *   recover: the one-workgroup kernel, which runs behind the team kernel on the same stream anyway, also samples
 *     every team cloud whose row starts with -1 (index-exact, counted in sn_wait_report);
 *   nowait: no teams, every cloud on one workgroup (as under graph capture). */
size_t sn_mds_workspace_bytes(int b, int n);
int sn_mds(const float *xyz, int b, int n, int m, const float *mean_mst_length,
           int *idx, void *workspace, size_t workspace_bytes, void *stream);
/* replaces MDS.gather_forward / MDS.gather_backward (MDS.cpp:54-113,138-139;
 *          kernels MDS_cuda.cu:29-79). feat[b,c,n], idx[b,m], out[b,c,m].
 * grad_feat is fully overwritten. */
int sn_gather_forward(const float *feat, const int *idx, int b, int c, int n,
                      int m, float *out, void *stream);
int sn_gather_backward(const float *grad_out, const int *idx, int b, int c,
                       int n, int m, float *grad_feat, void *stream);

/* ---------------------------------------------------------------------- p2i
 * replaces p2i_op.p2i_max_forward_gpu / p2i_max_backward_gpu
 *          (cuda/p2i_op/ext.cpp:8-9; p2i_max.h:145-232; functors :7-143)
 * points[npoints,2] pixel-space (row, col); feat[npoints,channels];
 * batch_inds[npoints]; background[batch,channels,h,w].
 * out/out_ids[batch,channels,h,w]; workspace holds the packed 64-bit image.
 * Ties between equal splat values resolve to the LOWEST point id (the
 * reference's GPU order is a race; its sequential CPU functor gives this). */
size_t sn_p2i_max_workspace_bytes(int batch, int channels, int h, int w);
int sn_p2i_max_forward(const float *points, const float *feat,
                       const int *batch_inds, const float *background,
                       int npoints, int channels, int batch, int h, int w,
                       float radius, float *out, int *out_ids, void *workspace,
                       size_t workspace_bytes, void *stream);
/* Several kernel radii over the same points / features / background in one pass
 * (ComputeDepthMaps calls p2i once per radius with identical inputs,
 * utils/p2i_utils.py:230-251): radii[nradii] is a HOST array, 1 <= nradii <= 4;
 * out / out_ids hold nradii [batch,channels,h,w] tensors, each equal to what
 * sn_p2i_max_forward returns for that radius: one after the other ([R,B,C,H,W],
 * image_major = 0) or interleaved per image ([B,R,C,H,W], image_major = 1: the layout
 * of the [B, len(radius_list), S, S] tensor ComputeDepthMaps returns, so that nothing
 * has to be transposed afterwards; radii <= 16 px).  background may be NULL = all zeros
 * (what ComputeDepthMaps passes; radii <= 16 px): no tensor is allocated, filled or read. */
size_t sn_p2i_max_multi_workspace_bytes(int npoints, int batch, int channels,
                                        int h, int w);
/* Test hook, not part of the reference surface: the renderer's two fp32 series in
 * u = r^2 / R^2 -- weight[i] ~ (cos(pi sqrt(u)) + 1) / 2 and slope[i] ~
 * sin(pi sqrt(u)) / (pi sqrt(u)) -- evaluated on the device for n values of u in
 * [0, 1]; the tests pin the error bounds the forward's decision band relies on. */
int sn_p2i_series(const float *u, int n, float *weight, float *slope, void *stream);
int sn_p2i_max_forward_multi(const float *points, const float *feat,
                             const int *batch_inds, const float *background,
                             int npoints, int channels, int batch, int h, int w,
                             const float *radii, int nradii, int image_major,
                             float *out, int *out_ids, void *workspace,
                             size_t workspace_bytes, void *stream);
/* points_grad[npoints,2], feat_grad[npoints,channels],
 * background_grad[batch,channels,h,w] are fully overwritten.
 * batch_inds: the forward's batch_inds, or NULL (the reference's backward does not
 * receive it; without it every image plane is searched for the point's wins). */
size_t sn_p2i_max_backward_workspace_bytes(int batch, int channels, int h, int w);
int sn_p2i_max_backward(const float *out_grad, const int *out_ids,
                        const float *points, const float *feat,
                        const int *batch_inds, int npoints, int channels,
                        int batch, int h, int w, float radius,
                        float *points_grad, float *feat_grad,
                        float *background_grad, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Backward of nradii splats that share points / features (the gradients of the radii
 * are summed, which is what autograd does with the reference's per-radius calls).
 * out_grad / out_ids: nradii [batch,channels,h,w] tensors in the layout of the forward
 * (image_major as there); background_grad may be NULL (not wanted).  Pixel-centric:
 * every pixel adds its fp32 terms to its winner in 64-bit fixed point (integer atomics),
 * so the sums are bit-reproducible.  The step is 2^(ilogb(m) - 43), m = max|out_grad| *
 * max(1, max|feat| * pi / (2 min(radii)) * 1.01) over the finite values: a gradient of n
 * terms is their exact sum to within n 2^-44 m, rounded once to fp32.  Non-finite terms
 * are not added: a gradient with a NaN term, or with both a +inf and a -inf term, is NaN,
 * one with only infinities of one sign is that infinity (the fp32 sum's result, in any
 * order).  The workspace holds 8 bytes and one class byte per output entry. */
size_t sn_p2i_max_backward_multi_workspace_bytes(int npoints, int channels);
int sn_p2i_max_backward_multi(const float *out_grad, const int *out_ids,
                              const float *points, const float *feat,
                              int npoints, int channels, int batch, int h, int w,
                              const float *radii, int nradii, int image_major,
                              float *points_grad, float *feat_grad,
                              float *background_grad,
                              void *workspace, size_t workspace_bytes,
                              void *stream);
/* replaces p2i_op.p2i_sum_forward_gpu / p2i_sum_backward_gpu
 *          (cuda/p2i_op/ext.cpp:6-7; p2i_sum.h:133-214; functors :7-131)
 * out must hold a copy of background on entry (the reference clones it,
 * p2i_sum.h:147); it is accumulated in place. */
int sn_p2i_sum_forward(const float *points, const float *feat,
                       const int *batch_inds, int npoints, int channels,
                       int batch, int h, int w, float radius, float *out,
                       void *stream);
int sn_p2i_sum_backward(const float *out_grad, const float *points,
                        const float *feat, const int *batch_inds, int npoints,
                        int channels, int batch, int h, int w, float radius,
                        float *points_grad, float *feat_grad, void *stream);

/* float64 tensors: the reference dispatches its functors on float and double (p2i_max.h:177,218,
 * p2i_sum.h:162,201) and its own test is a float64 gradcheck (cuda/p2i_op/p2i_test.py:23-35).  Same
 * semantics as the fp32 entry points above (lowest point id on equal values), simple atomics-based
 * kernels -- the rendering path of SpareNet itself is fp32. */
size_t sn_p2i_f64_workspace_bytes(int batch, int channels, int h, int w);
int sn_p2i_max_forward_f64(const double *points, const double *point_features, const int *batch_inds,
                           const double *background, int npoints, int channels, int batch, int h, int w,
                           double kernel_radius, double *out, int *out_point_ids, void *workspace,
                           size_t workspace_bytes, void *stream);
int sn_p2i_max_backward_f64(const double *out_grad, const int *out_point_ids, const double *points,
                            const double *point_features, int npoints, int channels, int batch, int h,
                            int w, double kernel_radius, double *points_grad, double *point_features_grad,
                            double *background_grad, void *stream);
int sn_p2i_sum_forward_f64(const double *points, const double *point_features, const int *batch_inds,
                           int npoints, int channels, int batch, int h, int w, double kernel_radius,
                           double *out, void *stream);
int sn_p2i_sum_backward_f64(const double *out_grad, const double *points, const double *point_features,
                            const int *batch_inds, int npoints, int channels, int batch, int h, int w,
                            double kernel_radius, double *points_grad, double *point_features_grad,
                            void *stream);

/* ---------------------------------------------------------- EdgeConv k-NN graph
 * replaces knn() / get_graph_feature() of models/sparenet_generator.py:852-906 (GPU branch:
 * the un-vendored KNN_CUDA 0.2 wheel).  inner[b,n,n] = x^T x (a plain batched GEMM, computed
 * by the caller with rocBLAS / torch.bmm), xx[b,n] = |x_j|^2.  idx[b,n,k] (int64): the k
 * smallest  |x_j|^2 - 2 x_i.x_j  per row, ascending, equal scores by lower index (the point
 * itself comes first); k in {1, 2, 4, 8, 16, 20, 32}. */
int sn_knn_topk(const float *inner, const float *xx, int b, int n, int k,
                long long *idx, void *stream);
/* The same search as ONE kernel on the fp32 matrix cores, from x[b,c,n] directly: the score tiles
 * 2 x_i.x_j - |x_j|^2 live in the MFMA accumulators and every lane keeps the k best of its queries
 * in registers, so the [b,n,n] matrix is never written (knn_mfma.hip).  idx[b,n,k] as above, the
 * point itself first; 1 <= k <= 20.  workspace: sn_knn_workspace_bytes(b, n) (the squared norms). */
size_t sn_knn_workspace_bytes(int b, int n);
int sn_knn(const float *x, int b, int c, int n, int k, long long *idx,
           void *workspace, size_t workspace_bytes, void *stream);
/* x[b,c,n], idx[b,n,k] -> out[b,2c,n,k]: out[:, ch] = x[idx] - x, out[:, c + ch] = x
 * (cat((feature - x, x), dim=3).permute(0, 3, 1, 2), :899-905); backward: grad_x[b,c,n]. */
int sn_graph_feature_forward(const float *x, const long long *idx, int b, int c,
                             int n, int k, float *out, void *stream);
size_t sn_graph_feature_backward_workspace_bytes(int b, int n, int k);
int sn_graph_feature_backward(const float *grad_out, const long long *idx, int b,
                              int c, int n, int k, float *grad_x, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ------------------------------------------------- PointNet feature pool (FPD)
 * The per-point MLP of Frechet/pointnet.py (STN3d and PointNetfeat: conv 3 -> 64 -> 128 -> 1024) and its max over
 * the points, fused (pointnet_pool.hip): xyz[b,n,3], trans[b,3,3] or NULL (identity), w1[64,3] b1[64], w2[128,64]
 * b2[128], w3[1024,128] b3[1024] (eval-mode batch norm already folded into them by the caller), out[b,1024]:
 *   x' = x . trans            (x'_j = fmaf(x2, t2j, fmaf(x1, t1j, x0 * t0j)); skipped for NULL)
 *   h1 = relu(W1 x' + b1), h2 = relu(W2 h1 + b2)
 *   out[cloud, j] = act(max over the points of (W3 h2)[j] + b3[j]),  act = ReLU if relu_last else identity
 * fp32 throughout; the K = 64 and K = 128 layers run on v_mfma_f32_32x32x2_f32: every sum is a k-ordered fp32 fmaf
 * chain (layers 1 and 2 start at the bias, layer 3 at 0; its bias and ReLU are applied once after the maximum, which
 * is bit-identical because both are monotone).  The [128, n] and [1024, n] activations never reach global memory;
 * tiles of 128 points are combined with a maximum, so the result does not depend on scheduling, on the order of the
 * points or on the batch a cloud is in.  Inputs are expected to be finite (fmaxf drops a NaN, torch.max keeps it).
 * Plain stream-ordered launches: no workgroup waits for another, no wait policy, may be captured into a graph.
 * workspace: sn_pointnet_pool_workspace_bytes(b, n) (transposed weights and per-tile maxima; 0 for invalid sizes).
 * Refused with SN_EINVAL: a null pointer (other than trans), b < 1, n < 1 or n > 2^20, a workspace too small. */
size_t sn_pointnet_pool_workspace_bytes(int b, int n);
int sn_pointnet_pool_forward(const float *xyz, const float *trans, const float *w1, const float *b1,
                             const float *w2, const float *b2, const float *w3, const float *b3,
                             int relu_last, int b, int n, float *out, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ------------------------------------------------------- depth-map projection
 * The per-view glue of ComputeDepthMaps.forward (utils/p2i_utils.py:211-228 and the NDC ->
 * pixel rescale of cuda/p2i_op/__init__.py:117-121) fused into two small kernels each way:
 * data[npoints,3] (all batch elements), matrix16 = P@V row major (HOST array), extent =
 * image_size - 1.  Outputs: pixel[npoints,2] (row, col) for sn_p2i_max_forward[_multi],
 * z[npoints] (projected depth), zminmax[2] (device scratch, order-preserving bits of the
 * global min / max of z), feat[npoints] = 1 - (z - zmin) / (zmax - zmin).
 * Backward: g_pixel / g_feat may be NULL; workspace32 = 32 bytes of device scratch;
 * includes the gradient paths through zmin / zmax as torch's autograd does. */
int sn_depth_project_forward(const float *data, long npoints, const float *matrix16,
                             float extent, float *pixel, float *z,
                             unsigned *zminmax, float *feat, void *stream);
int sn_depth_project_backward(const float *data, long npoints, const float *matrix16,
                              float extent, const float *z, const unsigned *zminmax,
                              const float *g_pixel, const float *g_feat,
                              void *workspace32, float *g_data, void *stream);

/* The same for up to 8 views at once (the views of a ComputeDepthMaps sweep become part of the batch:
 * pixel / z / feat are [nviews, npoints], zminmax [nviews, 2], normalisation per view as in the reference;
 * g_data [npoints, 3] receives the sum over the views).  matrices16: nviews x 16 host floats.
 * workspace: 32 bytes per view.  The single-view pair above equals these calls with nviews = 1 (the same
 * kernels, launched with grid caps of its own). */
int sn_depth_project_forward_views(const float *data, long npoints, const float *matrices16, int nviews,
                                   float extent, float *pixel, float *z, unsigned *zminmax, float *feat,
                                   void *stream);
int sn_depth_project_backward_views(const float *data, long npoints, const float *matrices16, int nviews,
                                    float extent, const float *z, const unsigned *zminmax,
                                    const float *g_pixel, const float *g_feat, void *workspace,
                                    float *g_data, void *stream);

/* ----------------------------------------------------------------- gridding
 * replaces gridding.forward / backward (cuda/gridding/gridding_cuda.cpp:44-67,
 *          94-95; gridding.cu:29-211, 213-335).  ptcloud[b,npts,3] already
 *          scaled; bounds are [-scale/2, scale/2-1] per axis as
 *          cuda/gridding/__init__.py:16-19 passes them.
 * grid[b,scale^3] fully overwritten; weights[b,npts,8,3]; indexes[b,npts,8].
 * scale must be even and 2 <= scale <= 1024 (scale^3 vertices stay inside an int); both
 * entry points refuse any other scale.  indexes holds the raw vertex index of every corner; a
 * corner whose index is outside [0, scale^3) contributes nothing, forward and backward. */
int sn_gridding_forward(const float *ptcloud, int b, int npts, int scale,
                        float *grid, float *weights, int *indexes,
                        void *stream);
/* The same with the reference module's padding rule done in the kernel: rows whose three
 * (already scaled) coordinates sum to zero are padding and contribute nothing
 * (cuda/gridding/__init__.py:41-47 filters them per sample on the host); their weights
 * are written as 0 and their indexes as -1, so the backward gives them a zero gradient. */
int sn_gridding_forward_padded(const float *ptcloud, int b, int npts, int scale,
                               float *grid, float *weights, int *indexes,
                               void *stream);
int sn_gridding_backward(const float *grad_grid, const float *weights,
                         const int *indexes, int b, int npts, int nverts,
                         float *grad_ptcloud, void *stream);
/* replaces gridding_distance.forward (cuda/gridding_loss/gridding_distance_cuda.cpp:
 *          forward -> gridding_distance.cu:179-212, kernel :29-177): integer bounds
 *          [min, max] per axis, grid[b, nverts, 8] with nverts = len_x len_y len_z (one
 *          accumulator per vertex and corner role), weights[b,npts,8,3], indexes[b,npts,8]
 *          (slot = vertex * 8 + corner).  gridding_distance.backward (:307-329) is
 *          sn_gridding_backward with nverts * 8 slots (grad kernel :214-314). */
int sn_gridding_dist_forward(const float *ptcloud, int b, int npts, int min_x,
                             int max_x, int min_y, int max_y, int min_z, int max_z,
                             float *grid, float *weights, int *indexes,
                             void *stream);
/* replaces gridding.rev_forward / rev_backward (gridding_cuda.cpp:69-91,96-97;
 *          gridding_reverse.cu:30-122, 124-236). grid[b,scale,scale,scale]. */
int sn_gridding_reverse_forward(const float *grid, int b, int scale,
                                float *ptcloud, void *stream);
/* ptcloud = the raw rev_forward output (what GriddingReverseFunction saves,
 * cuda/gridding/__init__.py:55), not the module's rescaled one. */
int sn_gridding_reverse_backward(const float *grad_ptcloud, const float *grid,
                                 const float *ptcloud, int b, int scale,
                                 float *grad_grid, void *stream);

/* --------------------------------------------------- cubic feature sampling
 * replaces cubic_feature_sampling.forward / backward
 *          (cuda/cubic_feature_sampling/cubic_feature_sampling_cuda.cpp:36-61;
 *           cubic_feature_sampling.cu:29-133, 135-205).
 * ptcloud[b,npts,3] in voxel space; feat[b,c,scale^3];
 * out[b,npts,(2ns)^3,c]; idx[b,npts,(2ns)^3]; grad_feat fully overwritten. */
int sn_cubic_forward(const float *ptcloud, const float *feat, int b, int npts,
                     int c, int scale, int ns, float *out, int *idx,
                     void *stream);
int sn_cubic_backward(const float *grad_out, const int *idx, int b, int npts,
                      int c, int scale, int ns, float *grad_feat,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARENET_HIP_H */
