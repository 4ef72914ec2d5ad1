# host/tests/map_refresh.mk -- test_map_refresh: the mirror of the map-point refresh (my_slam/vo/map_refresh.h), written against
# the reference-shaped headers and linked to libmvo_hip.so only (tests/test_map_refresh_host.py runs it on the MI355X and, with
# the emulated build in front of the library search path, on the CPU).
#   make -C host/tests -f map_refresh.mk
include Makefile
map_refresh: test_map_refresh
test_map_refresh: test_map_refresh.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_map_refresh.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := map_refresh
.PHONY: map_refresh
