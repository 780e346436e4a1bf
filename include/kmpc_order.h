/*
 * include/kmpc_order.h -- the ordered leader search: car following and lanes at fleet scale.
 *
 * An extension of the C ABI of include/kmpc.h, exported from the same library and under the same conventions (return codes, kmpc_last_error,
 * caller-owned buffers, `stream` a hipStream_t passed as void*).  The lists of entry points of include/kmpc.h, include/kmpc_follow.h,
 * include/kmpc_lanes.h and include/kmpc_range.h and the ABI version do not change; the four entry points below are this header's.
 *
 * kmpc_follow_fleet and kmpc_lane_step_fleet find every vehicle's neighbours by an exact pair search, O(B^2): cheap at a few thousand vehicles,
 * tens of milliseconds at a quarter of a million.  Their searches run along one dimension.  Order the fleet once per period by (path,
 * arclength): a vehicle's leader is then its successor, and the lane searches are look-ups in per-lane tables of the next occupied position,
 * O(B log B) in all.  The pair searches stay the specification: the entry points below give their outputs bit for bit, ties included.
 */
#ifndef KMPC_ORDER_H
#define KMPC_ORDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* THE ORDER of a fleet: a permutation of 0 ... B-1, a function of s_along, speed, path_id and present alone.  USABLE, AHEAD are
 * include/kmpc_follow.h's words, BEHIND is include/kmpc_lanes.h's.  The usable vehicles come first, sorted by
 *     1  path_id ascending (0 without path_id),
 *     2  arclength ascending, -0.0 ordered as +0.0,
 *     3  among equal arclengths, index DESCENDING;
 * the vehicles that are not usable come last, in ascending index.  In this order "j is AHEAD of b" is exactly "j is usable, on b's path and at
 * a later position", and BEHIND is the mirror.  Any finite arclength orders correctly -- negative, huge, subnormal -- and any path_id in
 * 0 ... 2^31 - 1.
 *
 * THE TIE RULE  the one place where "the successor" is not the answer.  The pair search takes the smallest ROUNDED difference and, among equal
 * rounded differences, the lowest j.  Along the order the rounded difference of the candidates never decreases, so the winner is the lowest
 * index in the RUN of in-band candidates that share the first in-band candidate's rounded difference: that candidate's group of equal
 * arclengths, and the few neighbouring arclengths whose difference rounds to the same value (when the difference lies in a higher binade than
 * the arclengths).  A candidate whose difference is +inf ends the search without a winner.
 *
 * kmpc_order_bytes        the size of `workspace` for the calls below; lanes_max 0 ... 32 is the number of lanes the lane tables cover (0: none,
 *                         enough for kmpc_order_fleet).  A host function, monotone in both arguments; 0 for B == 0.  KMPC_ERR_ARG for B < 0,
 *                         lanes_max outside 0 ... 32 or a NULL bytes_out.
 * kmpc_order_fleet        order_out [B] int32 DEVICE: THE ORDER.  count_out [1] int32 DEVICE or NULL: the number of usable vehicles.  s_along,
 *                         s_stride, speed, speed_stride, path_id, present: as in kmpc_follow_fleet.  workspace: DEVICE, at least
 *                         kmpc_order_bytes(B, 0) bytes, 256-byte aligned, written and read by this call only.
 *                         A stable radix sort of (path id, order-preserving image of the arclength) from descending index: per digit
 *                         per-workgroup counts, one scan, a stable scatter ranked by ballots; digits the whole fleet shares are skipped, decided
 *                         on the device.  A few dozen launches whatever B is.
 * kmpc_order_follow_fleet kmpc_follow_fleet's arguments in its order, then `order` [B] int32 DEVICE.  With kmpc_order_fleet's order for the same
 *                         s_along, speed, path_id and present: kmpc_follow_fleet's v_cap_out, gap_out, leader_out and every word of stat, bit for
 *                         bit.  One launch, no workspace.
 * kmpc_order_lane_step_fleet  kmpc_lane_step_fleet's arguments in its order, then `order`, lanes_max (0 ... 32), workspace (at least
 *                         kmpc_order_bytes(B, lanes_max) bytes) and workspace_bytes.  With kmpc_order_fleet's order for the same inputs:
 *                         kmpc_lane_step_fleet's v_cap_out, occ_out, every word of rec, gap_out, leader_out and nbr_out, bit for bit.  The call
 *                         first builds, for lanes 0 ... lanes_max - 1, tables of the next and the previous position whose vehicle is usable and
 *                         has that lane's bit in occ_in; the five searches start from table entries and follow a tie run along the same links.
 *                         A search whose band has a bit at or above lanes_max walks position by position instead: always exact, fast for the
 *                         lanes the tables were sized for.  A search whose band is 0 finds nobody and walks nothing.  occ_in == occ_out is
 *                         refused as in kmpc_lane_step_fleet.
 * Properties:
 *   - No host synchronisation, no allocation, no host read of device data; no global atomic; every output is a function of the inputs alone
 *     and does not depend on launch geometry.
 *   - An `order` that is not kmpc_order_fleet's for the same inputs gives unspecified leaders but no out-of-range access: every entry is
 *     range-checked before it indexes anything, and an entry outside 0 ... B-1 ends the search it turns up in; as a position's own entry it
 *     leaves that position without a vehicle, whose outputs are then not written.
 *   - A NaN stays in its own vehicle; the kernels cannot refuse a row.
 *   - KNOWN COST LIMIT: a tie run is walked linearly.  A fleet standing at one single arclength costs what the pair search costs.
 * Argument checks before any device call (they answer on a machine without a GPU), all KMPC_ERR_ARG with text in kmpc_last_error(NULL):
 *   kmpc_order_fleet: B < 0, a stride < 1, workspace_bytes < kmpc_order_bytes(B, 0); with B > 0 a NULL s_along, speed, order_out or workspace.
 *   kmpc_order_follow_fleet: kmpc_follow_fleet's; with B > 0 a NULL order.
 *   kmpc_order_lane_step_fleet: kmpc_lane_step_fleet's; lanes_max outside 0 ... 32, workspace_bytes < kmpc_order_bytes(B, lanes_max); with B > 0
 *   a NULL order or workspace.
 * B == 0 succeeds without a launch.  Asynchronous on `stream`. */
int32_t kmpc_order_bytes(int32_t B, int32_t lanes_max, int64_t *bytes_out);   /* HOST */
int32_t kmpc_order_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed, int32_t speed_stride,
                         const int32_t *path_id, const uint8_t *present, int32_t *order_out, int32_t *count_out, void *workspace,
                         int64_t workspace_bytes, void *stream);
int32_t kmpc_order_follow_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed, int32_t speed_stride,
                                const int32_t *path_id, const uint8_t *present, const double *rows, const double *v_cap, double *v_cap_out,
                                double *gap_out, int32_t *leader_out, double *stat, const int32_t *order, void *stream);
int32_t kmpc_order_lane_step_fleet(int32_t device, int32_t B, int32_t k, double dt, const double *s_along, int32_t s_stride, const double *e_ct,
                                   int32_t e_stride, const double *speed, int32_t speed_stride, const int32_t *path_id, const uint8_t *present,
                                   const double *follow_rows, const double *lane_rows, const double *v_cap, double *v_cap_out,
                                   const uint32_t *occ_in, uint32_t *occ_out, double *rec, double *gap_out, int32_t *leader_out, double *nbr_out,
                                   const int32_t *order, int32_t lanes_max, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
