/*
 * ops/mds_plan.h -- which kernels one sn_mds call launches, of libsparenet_hip.so: the sampler's host dispatch as a
 * pure function of values.  sn_mds (sparenet_hip.h) reads its knobs, the device and the wait policy, asks the same
 * function and launches from its answer; the instance tables (register slots per lane -> compiled instance) exist
 * nowhere else.  tests/test_mds_plan.py sweeps it on the CPU, and its coverage test pins which instance every GPU case
 * of tests/mds_plan_cases.py reaches.  Conventions as in ops/fps.h; nothing here touches the device unless `cus` <= 0,
 * and `plan` is a HOST array.  SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_MDS_PLAN_H
#define SPARENET_HIP_OPS_MDS_PLAN_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Words of the plan.  A word that does not apply to the family is 0 (TEAM_G: 1). */
#define SN_MDS_PLAN_FAMILY 0        /* SN_MDS_FAMILY_* below */
#define SN_MDS_PLAN_INSTANCE 1      /* REGISTERS: mds_kernel's PPT (2, 20, 24); CLUSTERED: mds_clustered_kernel's P */
#define SN_MDS_PLAN_ZLDS 2          /* REGISTERS: coordinates kept in LDS (mds_kernel's ZLDS: 0, 1 or 2) */
#define SN_MDS_PLAN_STATIC_BS 3     /* REGISTERS: mds_kernel's compile-time workgroup size (1024, or 0 = run-time) */
#define SN_MDS_PLAN_THREADS 4       /* lanes of the one-workgroup-per-cloud launch (the grid is b workgroups) */
#define SN_MDS_PLAN_PPT 5           /* points per lane of that launch, ceil(n / threads) */
#define SN_MDS_PLAN_LDS_BYTES 6     /* dynamic LDS of that launch */
#define SN_MDS_PLAN_LDS_OPT_IN 7    /* the dynamic-LDS limit that launch opts in to (0: the default limit) */
#define SN_MDS_PLAN_TEAM_G 8        /* CLUSTERED: workgroups per team; 1 = no team launch, every team word below is 0 */
#define SN_MDS_PLAN_TEAM_SLOTS 9    /* teams of the team launch (its grid is TEAM_SLOTS x TEAM_G workgroups) */
#define SN_MDS_PLAN_TEAM_PG 10      /* register slots per lane a member needs */
#define SN_MDS_PLAN_TEAM_NW 11      /* waves per member (the launch has 64 x TEAM_NW lanes) */
#define SN_MDS_PLAN_TEAM_INSTANCE 12 /* mds_dense_team_kernel's PG >= TEAM_PG; a member owns INSTANCE x NW groups of 64 */
#define SN_MDS_PLAN_TEAM_LDS_BYTES 13 /* dynamic LDS of the team launch */
#define SN_MDS_PLAN_TEAM_LDS_OPT_IN 14 /* the limit it opts in to */
#define SN_MDS_PLAN_TEAM_EVERY_REGIME 15 /* 1: teams sample every cloud; 0: only clouds above the SN_MDS_RATIO cross-over */
#define SN_MDS_PLAN_TEAM_CTL_BYTES 16 /* bytes of the teams' control block the call zeroes */
#define SN_MDS_PLAN_WORKSPACE_LO 17 /* workspace bytes the call needs: the low 32 bits ... */
#define SN_MDS_PLAN_WORKSPACE_HI 18 /* ... and the rest */
#define SN_MDS_PLAN_WORDS 19

#define SN_MDS_FAMILY_REGISTERS 0   /* mds_kernel<INSTANCE, ZLDS, STATIC_BS>: one workgroup per cloud, state in registers */
#define SN_MDS_FAMILY_GENERIC 1     /* mds_kernel_generic: one workgroup per cloud, densities in the workspace */
#define SN_MDS_FAMILY_CLUSTERED 2   /* cloud sort, mds_dense_team_kernel<TEAM_INSTANCE> when TEAM_G >= 2, then
                                       mds_clustered_kernel<INSTANCE> for the clouds no team took */

/* ------------------------------------------------------------ the sampler's dispatch
 * Writes the SN_MDS_PLAN_WORDS words above for a call sn_mds(xyz, b, n, ...) into plan[plan_words].
 *   cus          compute units of the device; <= 0: those of the current device (the only case that asks the runtime)
 *   g_cap        largest team size allowed, what SN_MDS_G supplies: 1..32, anything else means 32
 *   ratio_given  non-zero when SN_MDS_RATIO is set: the every-regime override of large clouds on large teams is off
 *   solo         non-zero forces one workgroup per cloud (wait policy nowait or latched, graph capture)
 * b, n >= 1, n < 2^22, plan_words >= SN_MDS_PLAN_WORDS; SN_EINVAL otherwise, and for a team geometry the kernels
 * cannot run (more than 10 register slots per lane or more than 1024 team workgroups: no input reaches it). */
int sn_mds_plan(int b, int n, int cus, int g_cap, int ratio_given, int solo, int *plan, int plan_words);

#ifdef __cplusplus
}
#endif

#endif
