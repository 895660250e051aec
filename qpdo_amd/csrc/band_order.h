/*
 * band_order.h -- a bandwidth-reducing variable order for the band direct solver (dev/band.inc, dev/band_wide.inc): reverse
 * Cuthill-McKee on the pattern of Q + A'A, computed on the host from the caller's CSC matrices, and the process-wide configuration
 * that says whether a workspace takes one (qpdo_amd_band_order_config, include/qpdo_amd_ext.h).  Pure host code: no HIP, a sibling
 * of csc_convert.c; tests/band_order_driver.c links this translation unit alone.
 *
 * The two public entry points (qpdo_amd_band_order, qpdo_amd_band_order_config) are declared in qpdo_amd_ext.h; what follows is
 * internal to libqpdo_amd.so.
 */
#ifndef QPDO_BAND_ORDER_H
#define QPDO_BAND_ORDER_H

#include <stddef.h>
#include <stdint.h>

#include "qpdo.h"
#include "qpdo_amd_ext.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(hidden)

/* reasons a configured order was not adopted (QPDOAmdBandOrderInfo.reason) */
enum {
    BAND_ORDER_REASON_NONE = 0,          /* adopted, or nothing configured */
    BAND_ORDER_REASON_NO_GAIN = 1,       /* RCM: b_ordered >= b_natural */
    BAND_ORDER_REASON_PARTITIONED = 2,   /* row-partitioned workspace */
    BAND_ORDER_REASON_COUPLING = 3,      /* QPDO_BAND_COUPLING > 0: a coupling row is wide under every order */
    BAND_ORDER_REASON_FUSED = 4,         /* the fused small-problem route */
    BAND_ORDER_REASON_LINSOLVE = 5,      /* QPDO_LINSOLVE is dense or pcg */
    BAND_ORDER_REASON_BORDER = 6         /* the workspace adopted a border of coupling variables (QPDO_BAND_BORDER): an arrowhead is wide under every order */
};
/* reasons a border of coupling variables was not adopted (QPDOAmdBandBorderInfo.reason; 2 .. 5 as above: the detection does not run) */
enum {
    BAND_BORDER_REASON_NONE = 0,         /* adopted, no border (c = 0), or the variable unset */
    BAND_BORDER_REASON_OVER = 1,         /* more border columns than QPDO_BAND_BORDER accepts */
    BAND_BORDER_REASON_PARTITIONED = 2,
    BAND_BORDER_REASON_COUPLING = 3,     /* QPDO_BAND_COUPLING > 0: the coupling-row mode keeps precedence */
    BAND_BORDER_REASON_FUSED = 4,
    BAND_BORDER_REASON_LINSOLVE = 5,
    BAND_BORDER_REASON_CORE = 6          /* the core is too short for the band solver's selection rule */
};

/* The half-bandwidth of the pattern of Q + A'A by band_detect's definition (dev/host_band.inc) -- the largest |i - j| over the
 * stored entries of Q (the stored triangle for stype != 0), the largest column span over the rows of A -- with variable v at
 * position oldnew[v]; oldnew NULL: the caller's order.  Returns -1 when the scratch cannot be allocated. */
long band_order_bandwidth(const cholmod_sparse *Q, const cholmod_sparse *A, const int32_t *oldnew);

/* One qpdo_setup's snapshot of the configuration for a workspace of n variables: *mode = QPDO_AMD_BAND_ORDER_NATURAL, _RCM or _GIVEN
 * (_ENV resolved through QPDO_BAND_ORDER); GIVEN: *newold = a malloc'd copy of the configured order (the caller frees it).  Returns 0,
 * or -1 with the reason in msg: a GIVEN order of another length, an unknown value of QPDO_BAND_ORDER, no memory. */
int band_order_snapshot(long n, int *mode, int32_t **newold, char *msg, size_t msg_len);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
