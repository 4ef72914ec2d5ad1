# host/tests/local_map.mk -- test_local_map: the mirror of the second search of a tracked frame (my_slam/vo/local_map.h), written
# against the reference-shaped headers and linked to libmvo_hip.so only (tests/test_local_map_host.py runs it on the MI355X and,
# with the emulated build in front of the library search path, on the CPU).
#   make -C host/tests -f local_map.mk
include Makefile
local_map: test_local_map
test_local_map: test_local_map.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_local_map.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := local_map
.PHONY: local_map
