/* Shared by the host half (rn_resize_host.c) and the kernel (rn_resize.hip) of the device resize. */
#ifndef RN_RESIZE_H
#define RN_RESIZE_H

#define RN_RS_DESC 12          /* 32-bit words of one image's descriptor (layout: rn_resize_host.c) */
#define RN_RS_MAX_SIDE 16384u  /* image sides and `resize` */
#define RN_RS_MAX_CROP 2048u   /* 3 * crop <= 256 threads x RN_RS_ACC accumulators */
#define RN_RS_MAX_SCALE 64u    /* source side / resized side */
#define RN_RS_ACC 24           /* accumulators a thread keeps: columns x rows of a band */

#endif
