/* tools/orb_ref/cu: stand-in for <thrust/system/cuda/execution_policy.h>; nothing of it is used below THRUST_VERSION 100800.  TEST INFRASTRUCTURE. */
