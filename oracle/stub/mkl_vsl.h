/* mkl_vsl.h -- TEST INFRASTRUCTURE ONLY.  Our own, deliberately empty header.
 *
 * The reference's rand.h:8 includes Intel MKL's mkl_vsl.h for the generator
 * behind rand.cpp.  dec.cpp includes rand.h only for the prototype of
 * rand_int(); it names no VSL type or function itself.  rand.cpp is not
 * compiled into oracle/_ref/librefdec.so (oracle/ref_dec_harness.cpp defines
 * rand_int), so this stand-in needs no contents and changes no arithmetic. */
