# tests/sim/init_finish.mk -- TEST AID built by tests/test_init_finish_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_init.so = the objects of libmvo_sim.so (Makefile) plus csrc/init_host.cpp, the host side of
# the finish of the monocular initialisation, compiled for x86 against hip_emu/ by the same pattern rule.
#   make -C tests/sim -f init_finish.mk _build/libmvo_sim_init.so
include Makefile
INIT_OBJ := $(FULL_OBJ) _build/full/init_host.cpp.o
_build/libmvo_sim_init.so: $(INIT_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
_build/full/init_host.cpp.o _build/full/track_kernels.hip.o: $(CSRC)/h_wave.h $(CSRC)/hd_wave.h $(CSRC)/init_wave.h
