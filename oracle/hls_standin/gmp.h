/* gmp.h -- stand-in: the reference includes <gmp.h> only to work round an old Vivado HLS header bug; nothing of it is used. */
#ifndef HLS_STANDIN_GMP_H
#define HLS_STANDIN_GMP_H
#endif
