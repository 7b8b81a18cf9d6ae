# The flame_agg_reduce_mx validation driver under ASan + UBSan: the Makefile's library rule, variables
# and flags (included unchanged), plus this one driver's build and run rules.  Run from this directory:
#     make -f mx_driver.mk OUT=<dir> run-mx_driver
# Sharing $(OUT) with the Makefile's drivers shares the one host-sanitized library build.
include Makefile

$(OUT)/mx_driver: $(ROOT)/tests/abi_asan/mx_driver.c $(OUT)/libflame_amd_asan.so
	$(CLANG) -O1 -g $(SAN) -I$(ROOT)/include -o $@ $< -L$(OUT) -l:libflame_amd_asan.so -Wl,-rpath,$(OUT)

run-mx_driver: $(OUT)/mx_driver
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 $(OUT)/mx_driver

.PHONY: run-mx_driver
