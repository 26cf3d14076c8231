/* grt_work_order.h -- which work item a workgroup of a line-kernel launch takes: the one statement of the mapping, for the
 * kernels (decode_work, gas_optics_dev.h) and, as plain C, for the host (grt_work_order, grt_gas_launch.c).
 *
 * A launch has ngroups "groups" -- one (cell tile, line slice) each -- of per_group = layers x columns workgroups that
 * all read the same slice of the line store.  Work items are numbered group-major, the (layer, column) index `rem`
 * varying fastest, and workgroup b takes item b.  The hardware deals workgroup ids round-robin to the 8 XCDs, so XCD x
 * gets the items x, x + 8, ... of EVERY group: an eighth of every tile, whatever the tile costs.  All XCDs walk the same
 * sequence of groups in step, and the ~128 workgroups resident on one (ids 8 k + x for 128 consecutive k: 1 017
 * consecutive items) belong to at most (1 015 + per_group)/per_group + 1 groups -- two wherever per_group >= 1 016, as in
 * every batched launch -- so an XCD's L2 holds one or two line slices at a time.  The price: each slice is read into
 * eight L2s, not one.  The groups are taken in spectral order: with every XCD on an eighth of every group there is
 * nothing left for a permutation of the groups to balance. */
#ifndef GRT_WORK_ORDER_H_
#define GRT_WORK_ORDER_H_

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRT_HOST_DEVICE __host__ __device__
#else
#define GRT_HOST_DEVICE
#endif

/* workgroup b of nb = ngroups*per_group -> its group and its (layer, column) index within the group */
GRT_HOST_DEVICE static inline void grt_work_order_map(unsigned nb, unsigned per_group, unsigned ngroups, unsigned b,
                                                      unsigned *group, unsigned *rem)
{
    (void)nb;
    (void)ngroups;
    *group = b/per_group;
    *rem = b - *group*per_group;
}

#endif
