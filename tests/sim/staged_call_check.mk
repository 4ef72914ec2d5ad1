# tests/sim/staged_call_check.mk -- TEST AID (never part of libmvo_hip.so): staged_call_check.cpp with csrc/staged_call.h, the
# frame scratch and packing of csrc/guided_match_host.h and hip_emu/, all under AddressSanitizer (with its leak check) and
# UndefinedBehaviorSanitizer, as one program.
#   make -C tests/sim -f staged_call_check.mk check
include Makefile
_build/staged_call_check: staged_call_check.cpp hip_emu/emu_runtime.cpp $(CSRC)/staged_call.h $(CSRC)/guided_match_host.h $(CSRC)/guided_knn2.h $(CSRC)/mvo_internal.h hip_emu/hip/hip_runtime.h
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ staged_call_check.cpp hip_emu/emu_runtime.cpp
check: _build/staged_call_check
	./_build/staged_call_check
.PHONY: check
