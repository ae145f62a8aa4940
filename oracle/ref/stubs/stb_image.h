/* stub: the reference harness reads no images */
