/* stub: the shim (oracle/ref/shim.h) supplies curandState, curand_init and curand_uniform */
