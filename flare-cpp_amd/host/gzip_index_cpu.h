// gzip_index_cpu.h -- the unit index of a gzip body (csrc/gzip_index.h) read on
// the host, and the serial model of the route fsg_inflate_units_batch takes
// for one body (include/flare_deflate_index_gpu.h).  No libz.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fsh_cpu_gzip_index's answer */
#define FSH_GZIP_INDEX_NONE 0     /* no FEXTRA, no RA subfield, or a head zlib refuses */
#define FSH_GZIP_INDEX_UNUSABLE 1 /* a broken chain, or a first RA subfield that misses a rule */
#define FSH_GZIP_INDEX_USABLE 2

/* The index of the gzip body in[0 .. n).  On USABLE: *chlen, *chcnt, and the
 * first byte of unit k in starts[k] for k < min(chcnt, starts_cap).  The other
 * answers leave the outputs alone.  starts may be NULL when starts_cap is 0. */
int fsh_cpu_gzip_index(const void *in, size_t n, uint32_t *chlen, uint32_t *chcnt, uint64_t *starts,
                       size_t starts_cap);

/* The routes of fsg_inflate_units_report, as the device must count one body. */
#define FSH_UNITS_ROUTE_PARALLEL 0 /* a usable index, every unit clean, the total within the slot */
#define FSH_UNITS_ROUTE_NO_INDEX 1 /* also: every raw or zlib body, and a body its wrapper decides */
#define FSH_UNITS_ROUTE_UNUSABLE 2
#define FSH_UNITS_ROUTE_MISMATCH 3 /* a unit that is not clean, or a total above the capacity */

/* format: FSG_INFLATE_*.  store = 1 models fsg_inflate_units_batch with a slot
 * of cap bytes, store = 0 fsg_inflate_units_lengths_batch (cap is not looked
 * at).  *units (may be NULL): the unit entries the body takes in the first
 * pass, CHCNT with a usable index, 0 for a body its wrapper decides, else 1.
 * The unit rules are those of fsh_cpu_inflate_unit run over the index. */
int fsh_cpu_inflate_units_route(uint32_t format, const void *in, size_t n, size_t cap, int store, uint32_t *units);

#ifdef __cplusplus
}
#endif
