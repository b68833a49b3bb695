# tests/cpp/attention_half_sim.mk — TEST CODE: the one rule of attention_half_sim, beside tests/cpp/Makefile (which it
# includes for CXX, CSRC, SIM_SAN, SIM_HDRS and sanitizer_probe), as attention_sim.mk.
#   attention_half_sim   csrc/attention.hip (with attention_half_kernel.hpp and attention_slice_walk.inc) compiled UNCHANGED
#                        with the host compiler over simt/, with the address and undefined-behaviour sanitizers, and driven
#                        through mi355_spmv_attention_create_half / _set_scale / _execute / _destroy: the program of
#                        tests/test_attention_half_sim_cpu.py, built on demand by it:
#                        make -C tests/cpp -f attention_half_sim.mk attention_half_sim
include Makefile

attention_half_sim: attention_half_sim.cpp $(CSRC)/attention.hip $(CSRC)/attention_half_kernel.hpp $(CSRC)/attention_slice_walk.inc $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
