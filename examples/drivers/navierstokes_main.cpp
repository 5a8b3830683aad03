// Steady Navier-Stokes driver on the MI355X path, written against the FEDD:: operator surface the way the reference's driver is
// (feddlib/problems/tests/steadyNavierStokes/main.cpp, "unstructured" branch): same XML parameter files, same call sequence
//   Domain(comm, dim) x 2 -> MeshPartitioner::readAndPartition -> buildP2ofP1Domain -> BCBuilder::addBC ->
//   NavierStokes(...) -> addBoundaries -> initializeProblem -> assemble -> setBoundariesRHS -> NonLinearSolver(type).solve ->
//   ExporterParaView.
// "Linearization" = FixedPoint | Newton and "Preconditioner Method" = "Monolithic" are built; NOX, Teko, the symmetric
// gradient and a multiplicative level combination are refused with the key named (NonLinearSolver, NavierStokes).
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/core/General/ExporterParaView.hpp"
#include "feddlib/problems/specific/NavierStokes.hpp"
#include "feddlib/problems/abstract/NonLinearProblem.hpp"
#include "feddlib/problems/Solver/NonLinearSolver.hpp"

void zeroDirichlet2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroDirichlet3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }
void inflowParabolic2D(double* x, double* res, double t, const double* parameters) {
    double H = parameters[1];
    res[0] = 4 * parameters[0] * x[1] * (H - x[1]) / (H * H);
    res[1] = 0.;
}
void inflowParabolic3D(double* x, double* res, double t, const double* parameters) {
    double H = parameters[1];
    res[0] = 16 * parameters[0] * x[1] * (H - x[1]) * x[2] * (H - x[2]) / (H * H * H * H);
    res[1] = 0.;
    res[2] = 0.;
}

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;

int main(int argc, char* argv[]) {
    typedef MeshPartitioner<SC, LO, GO, NO> MeshPartitioner_Type;
    typedef Teuchos::RCP<Domain<SC, LO, GO, NO> > DomainPtr_Type;
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "solutionNavierStokes.txt";
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile)) continue;
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::rcp(new Teuchos::Comm<int>(0, 1));
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        // the preconditioner's parameter file follows the method, as feddlib/problems/tests/stokes/main.cpp:171-179 does:
        // Diagonal / Triangular read parametersPrecBlock.xml beside the file given (or the file given, if it is that one)
        std::string precMethod = parameterListProblem->sublist("General").get("Preconditioner Method", "Monolithic");
        TEUCHOS_TEST_FOR_EXCEPTION(precMethod != "Monolithic" && precMethod != "Diagonal" && precMethod != "Triangular", std::logic_error,
                                   "\"Preconditioner Method\" = \"" << precMethod << "\" is not built (Monolithic, Diagonal and Triangular are; Teko and FaCSI are not)");
        if (precMethod != "Monolithic" && xmlPrecFile.find("parametersPrecBlock.xml") == std::string::npos) {
            const size_t slash = xmlPrecFile.find_last_of('/');
            xmlPrecFile = (slash == std::string::npos ? std::string() : xmlPrecFile.substr(0, slash + 1)) + "parametersPrecBlock.xml";
        }
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);

        int dim = parameterListProblem->sublist("Parameter").get("Dimension", 3);
        std::string discVelocity = parameterListProblem->sublist("Parameter").get("Discretization Velocity", "P2");
        std::string discPressure = parameterListProblem->sublist("Parameter").get("Discretization Pressure", "P1");
        std::string meshType = parameterListProblem->sublist("Parameter").get("Mesh Type", "structured");
        int volumeID = parameterListProblem->sublist("Parameter").get("Volume ID", 0);
        std::string bcType = parameterListProblem->sublist("Parameter").get("BC Type", "parabolic");
        TEUCHOS_TEST_FOR_EXCEPTION(meshType != "unstructured" && meshType != "structured", std::logic_error,
                                   "\"Mesh Type\" = \"" << meshType << "\" is not built (structured and unstructured are)");
        int m = parameterListProblem->sublist("Parameter").get("H/h", 5);
        TEUCHOS_TEST_FOR_EXCEPTION(discVelocity != "P2", std::logic_error, "this driver builds P2 / P1");

        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);

        Teuchos::RCP<Teuchos::Time> totalTime(Teuchos::TimeMonitor::getNewCounter("main: Total Time"));
        Teuchos::RCP<Teuchos::Time> buildMesh(Teuchos::TimeMonitor::getNewCounter("main: Build Mesh"));
        Teuchos::RCP<Teuchos::Time> solveTime(Teuchos::TimeMonitor::getNewCounter("main: Solve problem time"));
        DomainPtr_Type domainPressure, domainVelocity;
        int its = 0;
        {
            Teuchos::TimeMonitor totalTimeMonitor(*totalTime);
            {
                Teuchos::TimeMonitor buildMeshMonitor(*buildMesh);
                if (meshType == "structured") {
                    // the reference's "structured" branch (stokes/main.cpp:207-225): n = round(size^(1/dim)) blocks per direction,
                    // m = H/h cells per block, both domains from Domain::buildMesh with flags option 1
                    const int size = comm->getSize();
                    const int n = (int)(std::pow((double)size, 1. / dim) + 100 * 2.220446049250313e-16);
                    std::vector<double> x(dim, 0.0);
                    if (dim == 2) {
                        domainPressure.reset(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
                        domainVelocity.reset(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
                    } else {
                        domainPressure.reset(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
                        domainVelocity.reset(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
                    }
                    domainPressure->buildMesh(1, "Square", dim, discPressure, n, m, 0);
                    domainVelocity->buildMesh(1, "Square", dim, discVelocity, n, m, 0);
                } else {
                    domainPressure.reset(new Domain<SC, LO, GO, NO>(comm, dim));
                    domainVelocity.reset(new Domain<SC, LO, GO, NO>(comm, dim));
                    MeshPartitioner_Type::DomainPtrArray_Type domainP1Array(1);
                    domainP1Array[0] = domainPressure;
                    ParameterListPtr_Type pListPartitioner = Teuchos::sublist(parameterListAll, "Mesh Partitioner");
                    MeshPartitioner<SC, LO, GO, NO> partitionerP1(domainP1Array, pListPartitioner, "P1", dim);
                    partitionerP1.readAndPartition(volumeID);
                    domainVelocity->buildP2ofP1Domain(domainPressure);
                }
            }
            std::vector<double> parameter_vec(1, parameterListProblem->sublist("Parameter").get("MaxVelocity", 1.));
            Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
            if (!bcType.compare("parabolic")) parameter_vec.push_back(1.);
            else if (!bcType.compare("parabolic_benchmark")) parameter_vec.push_back(.41);
            else TEUCHOS_TEST_FOR_EXCEPTION(true, std::logic_error, "Select a valid boundary condition.");
            if (dim == 2) {
                bcFactory->addBC(zeroDirichlet2D, 1, 0, domainVelocity, "Dirichlet", dim);
                bcFactory->addBC(inflowParabolic2D, 2, 0, domainVelocity, "Dirichlet", dim, parameter_vec);
            } else {
                bcFactory->addBC(zeroDirichlet3D, 1, 0, domainVelocity, "Dirichlet", dim);
                bcFactory->addBC(inflowParabolic3D, 2, 0, domainVelocity, "Dirichlet", dim, parameter_vec);
            }
            bcFactory->addBC(dim == 2 ? zeroDirichlet2D : zeroDirichlet3D, 4, 0, domainVelocity, "Dirichlet", dim);   // flag of the obstacle

            NavierStokes<SC, LO, GO, NO> navierStokes(domainVelocity, discVelocity, domainPressure, discPressure, parameterListAll);
            domainVelocity->info();
            domainPressure->info();
            navierStokes.info();
            {
                Teuchos::TimeMonitor solveTimeMonitor(*solveTime);
                navierStokes.addBoundaries(bcFactory);
                navierStokes.initializeProblem();
                navierStokes.assemble();
                navierStokes.setBoundariesRHS();
                std::string nlSolverType = parameterListProblem->sublist("General").get("Linearization", "FixedPoint");
                NonLinearSolver<SC, LO, GO, NO> nlSolver(nlSolverType);
                nlSolver.solve(navierStokes);
            }
            (void)its;
            Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > exportSolutionV = navierStokes.getSolution()->getBlock(0);
            Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > exportSolutionP = navierStokes.getSolution()->getBlock(1);
            std::ofstream out(outFile);
            out << std::setprecision(17);
            // by global dof id (the maps' numbering: the identity for a mesh file, the reference's lattice ids for structured meshes)
            auto mapV = domainVelocity->getMapUnique();
            auto mapP = domainPressure->getMapUnique();
            for (size_t i = 0; i < exportSolutionV->getLocalLength(); ++i)
                out << (size_t)mapV->getGlobalElement((LO)(i / dim)) * dim + i % dim << " " << exportSolutionV->getData(0)[i] << "\n";
            const size_t off = exportSolutionV->getLocalLength();
            for (size_t i = 0; i < exportSolutionP->getLocalLength(); ++i)
                out << off + (size_t)mapP->getGlobalElement((LO)i) << " " << exportSolutionP->getData(0)[i] << "\n";
            if (parameterListAll->sublist("General").get("ParaViewExport", false)) {
                Teuchos::RCP<ExporterParaView<SC, LO, GO, NO> > exParaVelocity(new ExporterParaView<SC, LO, GO, NO>());
                Teuchos::RCP<ExporterParaView<SC, LO, GO, NO> > exParaPressure(new ExporterParaView<SC, LO, GO, NO>());
                exParaVelocity->setup("velocity", domainVelocity->getMesh(), domainVelocity->getFEType());
                exParaVelocity->addVariable(exportSolutionV, "u", "Vector", dim, domainVelocity->getMapUnique());
                exParaPressure->setup("pressure", domainPressure->getMesh(), domainPressure->getFEType());
                exParaPressure->addVariable(exportSolutionP, "p", "Scalar", 1, domainPressure->getMapUnique());
                exParaVelocity->save(0.0);
                exParaPressure->save(0.0);
            }
        }
        Teuchos::TimeMonitor::report(std::cout);
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
