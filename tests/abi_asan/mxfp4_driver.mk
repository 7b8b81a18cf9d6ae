# The flame_agg_reduce_mxfp4 validation driver under ASan + UBSan: the Makefile's library rule, variables
# and flags (included unchanged), plus this one driver's build and run rules.  Run from this directory:
#     make -f mxfp4_driver.mk OUT=<dir> run-mxfp4_driver
# Sharing $(OUT) with the Makefile's drivers shares the one host-sanitized library build.
include Makefile

$(OUT)/mxfp4_driver: $(ROOT)/tests/abi_asan/mxfp4_driver.c $(OUT)/libflame_amd_asan.so
	$(CLANG) -O1 -g $(SAN) -I$(ROOT)/include -o $@ $< -L$(OUT) -l:libflame_amd_asan.so -Wl,-rpath,$(OUT)

run-mxfp4_driver: $(OUT)/mxfp4_driver
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 $(OUT)/mxfp4_driver

.PHONY: run-mxfp4_driver
