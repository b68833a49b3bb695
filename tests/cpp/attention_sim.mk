# tests/cpp/attention_sim.mk — TEST CODE: the one rule of attention_sim, beside tests/cpp/Makefile (which it includes for
# CXX, CSRC, SIM_SAN, SIM_HDRS and sanitizer_probe).
#   attention_sim   csrc/attention.hip compiled UNCHANGED with the host compiler over simt/, with the address and
#                   undefined-behaviour sanitizers, and driven through mi355_spmv_attention_create / _set_scale /
#                   _execute / _destroy: the program of tests/test_attention_sim_cpu.py, built on demand by it:
#                   make -C tests/cpp -f attention_sim.mk attention_sim
include Makefile

attention_sim: attention_sim.cpp $(CSRC)/attention.hip $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
